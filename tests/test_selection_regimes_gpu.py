"""nw_topk_kernel<REGS, MAPPED, PAD> (topk.hip) in every row-length regime, behind each of its four public results:
ops.nw_topk, the second launch of ops.nw_knn (nw_knn_f32, MAPPED), the windowed search (nw_knn_window_f32, MAPPED + PAD) and
the half-precision search (nw_knn_f16, MAPPED).

The launchers choose the instantiation by the row length M alone: REGS = 16 / 32 / 64 keep the row in registers, REGS = 0
(M > 65536) re-reads it in every pass and has a body of its own for the histogram loads, the ordered compaction and the tie
cut-off.  For nw_topk M is N; for the searches it is (support tiles) x (candidate slots per tile), so the tile height is
pinned (NW_TILE_RS) and every case computes M itself and asserts the regime it means to hit BEFORE the launch.

The reference is never the code under test: torch.argsort(x.cpu(), dim=-1, descending=True, stable=True)[:, :k], values by a
gather on the same CPU tensor, everything compared with torch.equal.  For the searches x is the bank-route score matrix
(ops.nw_scores(q, s, support_cache=bank)) under the same tile height -- the contract of nw_knn's docstring.  The half form
has no score matrix to be bit-equal to: it is held to the conditions of test_knn_half_gpu._check, unchanged."""
import contextlib
import functools

import pytest
import torch

from test_knn_fused_gpu import _data, _fused_calls, dev, ops  # noqa: F401  (fixtures, the generator, the launch spy)
from test_knn_half_gpu import _case as _half_case, _check as _half_check, _search as _half_search
from test_knn_window_gpu import _window_calls

pytestmark = pytest.mark.gpu

NEG_INF = float("-inf")
# The row lengths up to which launch_topk and launch_topk_candidates (topk.hip) take nw_topk_kernel<16>, <32> and <64>
# (16, 32 and 64 elements in the registers of each of 1024 threads); longer rows take <0>.
REGS16_MAX, REGS32_MAX, REGS64_MAX = 16384, 32768, 65536
TK_THREADS = 1024


def _regs(M):
    return 16 if M <= REGS16_MAX else 32 if M <= REGS32_MAX else 64 if M <= REGS64_MAX else 0


def _stable_order(x):
    return torch.argsort(x.cpu(), dim=-1, descending=True, stable=True)


# ------------------------------------------------------------------------------------------------------------- 1. nw_topk
# both sides of every boundary; 65537 leaves the highest threads of REGS = 0 with empty ranges; 100003 has a ragged last
# per-thread range and several 8192-element histogram trips
TOPK_N = [(16384, 16), (16385, 32), (32768, 32), (32769, 64), (65536, 64), (65537, 0), (100003, 0), (200000, 0)]
TOPK_K = [1, 64, 65, 1000, 1024]          # 64 | 65: the one-wave sort and the LDS bitonic sort


@functools.lru_cache(maxsize=None)
def _random_rows(N):
    """Three rows of the suite's scores (like -distance: one sign, one exponent) with their full stable order."""
    g = torch.Generator().manual_seed(3 * 131 + N)
    s = torch.randn(3, N, generator=g) * 3 - 30
    return s.cuda(), s, _stable_order(s)


@pytest.mark.parametrize("k", TOPK_K)
@pytest.mark.parametrize("N,regs", TOPK_N)
def test_topk_random_rows(dev, ops, N, regs, k):
    assert _regs(N) == regs
    s_dev, s, order = _random_rows(N)
    idx, vals = ops.nw_topk(s_dev, k, return_values=True)
    ref = order[:, :k]
    assert torch.equal(idx.cpu(), ref)
    assert torch.equal(vals.cpu(), torch.gather(s, 1, ref))


def _tie_matrix(N, k):
    """Four rows whose k-th largest value is shared, built without a random draw that depends on k.
    0: a constant row: the first k indices.
    1: seven distinct integers: the tie group of the threshold spans every thread and every wave.
    2: k-1 strictly greater (distinct) elements at the very end of the row -- inside the last ceil(N/1024) positions, the
       range of the last live thread of REGS = 0, as far as that many fit -- and ONE tied value everywhere else: the tie
       cut-off must take index 0 and nothing else of the group.
    3: the tied value stands at index 0 and in the last 2 ceil(N/1024) positions only; n_eq = min(k, 1 + ceil(N/1024)) of the
       group make it (index 0 and the first of the tail: the cut falls inside the tail, past a thread-range boundary),
       k - n_eq distinct greater elements are spread over the row, everything else is smaller."""
    per = -(-N // TK_THREADS)
    x = torch.empty(4, N)
    x[0] = 1.5
    x[1] = torch.randint(-3, 4, (N,), generator=torch.Generator().manual_seed(N)).float()
    x[2] = -7.0
    if k > 1:
        x[2, N - (k - 1):] = torch.arange(k - 1).float() - 6.0
    x[3] = -5.0
    x[3, 0] = 2.0
    x[3, N - 2 * per:] = 2.0
    n_gt = k - min(k, 1 + per)
    if n_gt:
        stride = (N - 2 * per - 1) // n_gt
        assert stride >= 1
        at = 1 + stride * torch.arange(n_gt)
        assert int(at.max()) < N - 2 * per
        x[3, at] = 3.0 + torch.arange(n_gt).float()
    return x


@pytest.mark.parametrize("k", TOPK_K)
@pytest.mark.parametrize("N,regs", TOPK_N)
def test_topk_threshold_ties(dev, ops, N, regs, k):
    assert _regs(N) == regs
    x = _tie_matrix(N, k)
    idx, vals = ops.nw_topk(x.to(dev), k, return_values=True)
    ref = _stable_order(x)[:, :k]
    assert ref[0].tolist() == list(range(k)) and ref[2, k - 1].item() == 0 and 0 in ref[3].tolist()    # (of the construction)
    assert torch.equal(idx.cpu(), ref)
    assert torch.equal(vals.cpu(), torch.gather(x, 1, ref))


def _specials(N):
    """Three rows of +NaN and -NaN, +-inf, +-0.0 interleaved, denormals and a mixed-sign wide-range remainder.  Row 0 has 900
    positive elements, so that k = 1000 and 1024 cut inside the 100 zeros (one image: index order); row 1 has 400, so that
    they run through the zeros and the negative denormals into the smallest negatives; row 2 keeps the remainder as it is
    (half of it positive) and is rolled, like row 1, so that the specials stand elsewhere."""
    g = torch.Generator().manual_seed(3)
    base = torch.randn(3, N, generator=g) * torch.logspace(-20, 20, N)
    for r, n_pos in ((0, 900), (1, 400)):
        keep = torch.randperm(N, generator=g)[:n_pos]
        sign = torch.full((N,), -1.0)
        sign[keep] = 1.0
        base[r] = base[r].abs() * sign
    rows = []
    for r in range(3):
        x = base[r].clone()
        x[[3, N // 2, N - 1]] = float("nan")
        x.view(torch.int32)[[10, N // 3]] = -0x00400000                # 0xFFC00000: a NaN with the sign bit set
        x[20:60:4] = float("inf")
        x[21:61:4] = NEG_INF
        x[100:200:2] = -0.0
        x[101:201:2] = 0.0
        x[300:320] = 1e-40 * torch.arange(1, 21).float()               # denormals of both signs, the smallest one included
        x[320:340] = -1e-40 * torch.arange(1, 21).float()
        x.view(torch.int32)[340] = 1
        rows.append(torch.roll(x, r * 977))
    x = torch.stack(rows)
    assert int(x.isnan().sum()) == 15 and bool((x.view(torch.int32) == -0x00400000).any())
    assert bool(((x != 0) & (x.abs() < 1e-38)).any()), "the denormals are still there"
    return x


@pytest.mark.parametrize("N", [65537, 100003])
def test_topk_specials(dev, ops, N):
    assert _regs(N) == 0
    x = _specials(N)
    order = _stable_order(x)
    assert all(100 <= int(order[0, k - 1]) < 200 for k in (1000, 1024)), "row 0: the cut falls inside the zeros"
    assert bool((x[1, order[1, 999]] < 0) & (x[1, order[1, 999]] > -1e-10)), "row 1: past the zeros and the denormals"
    x_dev = x.to(dev)
    for k in TOPK_K:
        idx, vals = ops.nw_topk(x_dev, k, return_values=True)
        ref = order[:, :k]
        assert torch.equal(idx.cpu(), ref), k
        want, got = torch.gather(x, 1, ref), vals.cpu()
        assert torch.equal(got.isnan(), want.isnan()), k
        assert torch.equal(got[~want.isnan()], want[~want.isnan()]), k


# ---------------------------------------------------------------------------------------- 2. MAPPED: nw_knn in each regime
KNN_B, KNN_D = 5, 32


@contextlib.contextmanager
def _tile_height(monkeypatch, rs):
    """Pins the support-tile height (the score call follows the same knob) -> BS; restored on the way out."""
    from nwhead_amd import _lib
    from nwhead_amd.ops import _WS_BYTES
    monkeypatch.setenv("NW_SPLIT_ALWAYS", "1")
    monkeypatch.setenv("NW_TILE_RS", str(rs))
    _lib.sync_knobs()
    try:
        _WS_BYTES.clear()                      # sizes answered under another tile height
        yield 16 * rs
    finally:
        monkeypatch.delenv("NW_TILE_RS")
        _lib.sync_knobs()
        _WS_BYTES.clear()


def _cand_row_length(N, k, BS):
    """M of launch_topk_candidates: support tiles x cand_slots(k, BS) (fused_impl.h)."""
    return -(-N // BS) * ((min(k, BS) + 3) & ~3)


def _copies(N, BS):
    """40 rows for the copies of one bank row: three in the first tile, its last row and the first row of the next tile
    (neighbours across a tile boundary), one in each of 34 tiles spread evenly up to the last but one, two in the last tile."""
    tiles = -(-N // BS)
    rows = [1, 5, BS - 1, BS] + [(1 + j * (tiles - 3) // 33) * BS + (5 * j + 2) % BS for j in range(34)] + [N - 3, N - 1]
    assert rows == sorted(set(rows)) and len(rows) == 40 and (N - 3) // BS == tiles - 1 and rows[-3] // BS < tiles - 1
    return rows


LOO_ROW = 4321          # the bank row that query 1 is (the leave-one-out window of part 3)


@functools.lru_cache(maxsize=None)
def _bank(N, BS):
    """(q, s, bank, copies) of one shape, built once.  40 rows of s are copies of one row, and query 0 is that row with one
    coordinate moved by 1 (distance 1; every other row lies ~7 away): a tie group of 40 at the top of query 0, cut at
    k <= 32.  Query 1 is a bank row.

    The copies have to score bit-equal at every position of every tile.  Small integers make the dot products and their
    partial sums exact whatever the order of the summation (test_ties_keep_the_lowest_rows_in_order) -- but the tile
    epilogue forms x = acc K Cq + (|s|^2 c + |q|^2 c) with c = (log2 e)^2 (ScoreFactors, nw_internal.h), where the compiler
    is free to fuse a product into a sum for one register slot and not for another, so rows at different heights of a tile
    can round differently when a product is inexact.  Measured at 262276 rows on 128-row tiles: copies of a row of integers
    in [-3, 3] at distance 1 score -0.9999962 at 124 heights of every tile and -1.0000036 at heights 115, 119, 123 and 127
    (both well inside the 3e-5 of the scores; one value at every height of 32-row tiles) -- no tie group.
    Sixteen entries of +-1 and sixteen zeros: |s|^2 = 16 and q.s = 16 are powers of two, so |s|^2 c and acc K Cq are exact
    products, every fused and unfused form of the expression rounds once, at the same place, and the bits are the same
    at every height (measured: one value, both tile heights)."""
    from nwhead_amd import ops
    q, s = _data(torch.device("cuda:0"), KNN_B, N, KNN_D)
    copies = _copies(N, BS)
    assert LOO_ROW not in copies
    g = torch.Generator().manual_seed(N)
    at = torch.randperm(KNN_D, generator=g)
    row = torch.zeros(KNN_D)
    row[at[:16]] = torch.randint(0, 2, (16,), generator=g).float() * 2 - 1
    s[copies] = row.to(s.device)
    q[0] = row.to(s.device)
    q[0, at[16]] = 1.0
    assert float(row @ row) == 16.0 and float(q[0].cpu() @ row) == 16.0 and float((q[0].cpu() - row).norm()) == 1.0
    q[1] = s[LOO_ROW]
    return q, s, ops.SplitBank(s), copies


def _knn_case(ops, monkeypatch, rs, N, k, regs):
    with _tile_height(monkeypatch, rs) as BS:
        M = _cand_row_length(N, k, BS)
        if regs is not None:
            assert _regs(M) == regs, (M, _regs(M))
        assert N % 4 == 0
        q, s, bank, copies = _bank(N, BS)
        S = ops.nw_scores(q, s, support_cache=bank).cpu()
        ref = _stable_order(S)[:, :k]
        calls = _fused_calls(ops, monkeypatch)
        idx, val = ops.nw_knn(q, bank, k, return_values=True, support=s)
        assert calls == [(KNN_B, N, KNN_D, k)], "the fused search ran, not the score-matrix route"
        assert idx.dtype == torch.int64 and idx.shape == (KNN_B, k)
        assert torch.equal(idx.cpu(), ref)
        assert torch.equal(val.cpu(), torch.gather(S, 1, ref))
        assert idx[0].tolist() == copies[:k], "the lowest rows of the tie group, in ascending order"
        assert int(val[0].view(torch.int32).unique().numel()) == 1


# rs = 2 (BS = 32, 32 slots per tile at k = 32): M = N for whole tiles, + 28 empty slots with a ragged last tile of 4 rows.
# Both sides of the first and the last boundary of launch_topk_candidates; rs = 8 is the benchmark's tile height.
KNN_SHAPES = [(2, 16384, 16384, 16), (2, 16420, 16448, 32), (2, 32772, 32800, 64), (2, 65536, 65536, 64),
              (2, 65540, 65568, 0), (8, 262276, 65600, 0)]


@pytest.mark.parametrize("rs,N,M,regs", KNN_SHAPES)
def test_knn_candidate_row_in_each_regime(dev, ops, monkeypatch, rs, N, M, regs):
    assert _cand_row_length(N, 32, 16 * rs) == M
    _knn_case(ops, monkeypatch, rs, N, 32, regs)


@pytest.mark.parametrize("k", [1, 10])
def test_knn_fewer_slots_per_tile(dev, ops, monkeypatch, k):
    """The padded slot count follows k (4 and 12 slots per tile): the same bank on a shorter candidate row, whichever
    regime that is."""
    _knn_case(ops, monkeypatch, 2, 65540, k, None)


# -------------------------------------------------------------------------------- 3. MAPPED + PAD: the windowed search
def _masked_reference(S, k, lo, hi, exclude):
    """The stable argsort of the scores with everything outside the window at -inf; the slots past the admitted count are
    (-1, -inf).  All on the CPU."""
    cols = torch.arange(S.shape[1])
    keep = (cols >= lo[:, None]) & (cols < hi[:, None])
    if exclude:
        keep = ~keep
    Sm = S.masked_fill(~keep, NEG_INF)
    order = _stable_order(Sm)[:, :k]
    empty = torch.arange(k)[None, :] >= keep.sum(1)[:, None]
    return order.masked_fill(empty, -1), torch.gather(Sm, 1, order).masked_fill(empty, NEG_INF), keep.sum(1)


@pytest.mark.parametrize("exclude", [False, True], ids=["inside", "excluded"])
@pytest.mark.parametrize("rs,N,M,regs", [c for c in KNN_SHAPES if c[0] == 2])
def test_knn_window_in_each_regime(dev, ops, monkeypatch, rs, N, M, regs, exclude):
    k = 32
    with _tile_height(monkeypatch, rs) as BS:
        assert _cand_row_length(N, k, BS) == M and _regs(M) == regs
        q, s, bank, copies = _bank(N, BS)
        if not exclude:
            # the tie group, 33 of its copies admitted; 5 rows (the threshold is the empty key, most tiles are dead);
            # exactly k rows across a tile boundary; the whole bank; nothing
            win = [(copies[5], copies[37] + 1), (7 * BS + 3, 7 * BS + 8), (9 * BS - 10, 9 * BS + 22), (0, N), (777, 777)]
            counts = [copies[37] + 1 - copies[5], 5, k, N, 0]
            tied = copies[5:37]
        else:
            # the tie group without three of its copies; leave-one-out (query 1 is that row); three rows survive, all in the
            # last tile; the empty window: the whole bank; all but 5 rows
            win = [(copies[3], copies[6]), (LOO_ROW, LOO_ROW + 1), (0, N - 3), (777, 777), (7 * BS + 3, 7 * BS + 8)]
            counts = [N - (copies[6] - copies[3]), N - 1, 3, N, N - 5]
            tied = (copies[:3] + copies[6:])[:k]
        lo = torch.tensor([w[0] for w in win], device=dev)
        hi = torch.tensor([w[1] for w in win], device=dev)
        S = ops.nw_scores(q, s, support_cache=bank).cpu()
        ridx, rval, count = _masked_reference(S, k, lo.cpu(), hi.cpu(), exclude)
        assert count.tolist() == counts
        calls = _window_calls(monkeypatch)
        idx, val = ops.nw_knn(q, bank, k, return_values=True, support=s, row_window=(lo, hi), exclude=exclude)
        assert calls == [(KNN_B, N, KNN_D, k)], "the fused windowed search ran, not the masked score matrix"
        assert idx.dtype == torch.int64 and idx.shape == (KNN_B, k) and val.shape == (KNN_B, k)
        assert torch.equal(idx.cpu(), ridx)
        assert torch.equal(val.cpu(), rval)
        assert idx[0].tolist() == tied, "the lowest admitted rows of the tie group, in ascending order"
        if exclude:
            assert LOO_ROW not in idx[1].tolist() and bool((idx[1] >= 0).all())
            assert sorted(idx[2, :3].tolist()) == [N - 3, N - 2, N - 1] and idx[2, 3:].tolist() == [-1] * (k - 3)
        else:
            assert idx[4].tolist() == [-1] * k and bool((val[4] == NEG_INF).all())
            assert sorted(idx[2].tolist()) == list(range(9 * BS - 10, 9 * BS + 22))


# ------------------------------------------------------------------------------------------------- 4. the half form, once
def test_knn_half_form_regs32(dev, ops):
    """513 tiles of 128 supports (the half form's only tile height) x 32 slots: M = 16416, nw_topk_kernel<32, MAPPED> behind
    nw_knn_f16.  Conditions and reference of test_knn_half_gpu: fp64 scores of the rounded operands, 64 queries at a time."""
    B, N, d, k = 4, 65664, 192, 32
    M = _cand_row_length(N, k, 128)
    assert M == 16416 and _regs(M) == 32
    q, s, S = _half_case(B, N, d, "euclidean")
    idx, val = _half_search(ops, q, s, k, "euclidean", dev)
    _half_check(idx, val, S, k)
