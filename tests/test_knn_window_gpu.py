"""ops.nw_knn(row_window=...) / nw_knn_window_f32: the k best rows of a per-query row window of a prepared bank, kept or
excluded, without the (B,N) score matrix -- the candidate epilogue of the split-fp16 tile kernel turns the keys of the
rows a window does not admit into "no element" (fused_impl.h, tile_candidates), and the final selection pads a query that
has fewer than k rows with (-1, -inf) (topk.hip, PAD).

The reference is the parent's route with the mask applied by torch: nw_topk of the masked bank-route score matrix.  For
every query the first min(k, rows the window admits) slots equal the reference, rows and values, with torch.equal; the
remaining slots are (-1, -inf).  Like test_knn_fused_gpu.py, the exact cases run with and without NW_SPLIT_ALWAYS=1 (without
it the small shapes take nw_knn's score-matrix route with its torch mask), and one shape is fused without the switch."""
import pytest
import torch

import ws_poison
from test_knn_fused_gpu import _data, dev, ops, split_always  # noqa: F401  (fixtures and the generator, by import)

pytestmark = pytest.mark.gpu

NEG_INF = float("-inf")
TILE_HEIGHTS = (32, 64, 80, 96, 128, 160)
ALL_TILES = 1920          # a multiple of every tile height


def _window_calls(monkeypatch):
    """Counts the nw_knn_window_f32 launches (B, N, d, k of each): which route a call took."""
    from nwhead_amd import _lib
    lib = _lib.load()
    real = lib.nw_knn_window_f32
    calls = []

    class Spy:
        def __getattr__(self, name):
            if name == "nw_knn_window_f32":
                return lambda *a: (calls.append(a[11:15]), real(*a))[1]
            return getattr(lib, name)

    monkeypatch.setattr(_lib, "_lib", Spy())
    return calls


@pytest.fixture
def launches(monkeypatch):
    return _window_calls(monkeypatch)


def _admitted(N, lo, hi, exclude):
    cols = torch.arange(N, device=lo.device)
    inside = (cols >= lo[:, None]) & (cols < hi[:, None])
    return ~inside if exclude else inside


def _reference(ops, q, s, bank, k, lo, hi, exclude, kind="euclidean", ls=None):
    mask = _admitted(s.shape[0], lo, hi, exclude)
    S = ops.nw_scores(q, s, kind, ls, support_cache=bank).masked_fill(~mask, NEG_INF)
    ridx, rval = ops.nw_topk(S, k, return_values=True)
    return ridx, rval, mask.sum(1)


def _check(ops, q, s, bank, k, lo, hi, exclude, kind="euclidean", ls=None):
    """Every query, every slot: the valid ones against the reference, the rest (-1, -inf)."""
    idx, val = ops.nw_knn(q, bank, k, kind, ls, return_values=True, support=s, row_window=(lo, hi), exclude=exclude)
    ridx, rval, count = _reference(ops, q, s, bank, k, lo, hi, exclude, kind, ls)
    assert idx.dtype == torch.int64 and idx.shape == (q.shape[0], k) and val.shape == (q.shape[0], k)
    valid = torch.arange(k, device=idx.device)[None, :] < count[:, None]
    assert torch.equal(idx[valid], ridx[valid])
    assert torch.equal(val[valid], rval[valid])
    assert bool((idx[~valid] == -1).all()) and bool((val[~valid] == NEG_INF).all())
    assert torch.equal(ops.nw_knn(q, bank, k, kind, ls, support=s, row_window=(lo, hi), exclude=exclude), idx)
    return idx, val


def _class_windows(dev, B, N, C=16, seed=11):
    """The row ranges of C sorted classes under random query labels."""
    sy = (torch.arange(N) % C).sort().values.to(dev)
    qy = torch.randint(0, C, (B,), generator=torch.Generator().manual_seed(seed)).to(dev)
    return torch.searchsorted(sy, qy), torch.searchsorted(sy, qy, right=True)


def _tensor_pair(dev, pairs, B):
    lo = torch.tensor([pairs[b % len(pairs)][0] for b in range(B)], device=dev)
    hi = torch.tensor([pairs[b % len(pairs)][1] for b in range(B)], device=dev)
    return lo, hi


# ---- basic cases
@pytest.mark.parametrize("exclude", [False, True], ids=["inside", "excluded"])
@pytest.mark.parametrize("k", [1, 10, 32])
@pytest.mark.parametrize("B,N,d", [(37, 4100, 96), (130, 1000, 64), (256, 2048, 512)])
def test_class_windows_equal_the_masked_topk(dev, ops, split_always, launches, B, N, d, k, exclude):
    q, s = _data(dev, B, N, d)
    lo, hi = _class_windows(dev, B, N)
    _check(ops, q, s, ops.SplitBank(s), k, lo, hi, exclude)
    fused = split_always or B * N * d >= 2e8
    assert len(launches) == (2 if fused else 0), "the windowed search is fused exactly where the plain one is"


# ---- boundaries
@pytest.mark.parametrize("exclude", [False, True], ids=["inside", "excluded"])
def test_windows_at_tile_boundaries(dev, ops, split_always, launches, exclude):
    """Per query one of: strictly inside one tile (every height: a tile starts at 1920 and has at least 32 rows); ends on
    tile boundaries of every height; ends at N inside the ragged last tile (4100 is a multiple of no height); starts one
    row before / ends one row after a boundary; a single row; the first and the last row of the bank."""
    B, N, d = 37, 4100, 96
    q, s = _data(dev, B, N, d)
    pairs = [(ALL_TILES + 5, ALL_TILES + 20), (ALL_TILES, 2 * ALL_TILES), (4000, N), (4097, N), (ALL_TILES - 1, ALL_TILES + 1),
             (0, ALL_TILES), (ALL_TILES, N), (2000, 2001), (0, 1), (N - 1, N), (ALL_TILES - 40, ALL_TILES)]
    lo, hi = _tensor_pair(dev, pairs, B)
    for k in (1, 10, 32):
        _check(ops, q, s, ops.SplitBank(s), k, lo, hi, exclude)
    assert bool(launches) == split_always


# ---- degenerate windows
def test_degenerate_windows(dev, ops, split_always, launches):
    B, N, d, k = 37, 4100, 96, 10
    q, s = _data(dev, B, N, d)
    bank = ops.SplitBank(s)
    plain = ops.nw_knn(q, bank, k, return_values=True, support=s)
    at = torch.full((B,), 777, device=dev)
    zero, full = torch.zeros(B, dtype=torch.int64, device=dev), torch.full((B,), N, device=dev)
    # lo == hi
    idx, val = _check(ops, q, s, bank, k, at, at, False)
    assert bool((idx == -1).all()) and bool((val == NEG_INF).all())
    idx, val = _check(ops, q, s, bank, k, at, at, True)
    assert torch.equal(idx, plain[0]) and torch.equal(val.view(torch.int32), plain[1].view(torch.int32))
    # lo > hi is empty too
    idx, val = _check(ops, q, s, bank, k, at, at - 100, False)
    assert bool((idx == -1).all())
    # [0, N)
    idx, val = _check(ops, q, s, bank, k, zero, full, False)
    assert torch.equal(idx, plain[0]) and torch.equal(val.view(torch.int32), plain[1].view(torch.int32))
    idx, val = _check(ops, q, s, bank, k, zero, full, True)
    assert bool((idx == -1).all()) and bool((val == NEG_INF).all())
    # values outside [0, N] are clamped, never used as an address
    idx, val = ops.nw_knn(q, bank, k, return_values=True, support=s, row_window=(zero - 5, full + (1 << 30)))
    assert torch.equal(idx, plain[0]) and torch.equal(val.view(torch.int32), plain[1].view(torch.int32))
    assert bool(launches) == split_always


@pytest.mark.parametrize("k", [10, 32])
def test_fewer_rows_than_k(dev, ops, split_always, launches, k):
    """Windows of 3 rows: three valid slots, then (-1, -inf); some of them straddle a tile boundary of every height."""
    B, N, d = 37, 4100, 96
    q, s = _data(dev, B, N, d)
    starts = [0, 100, ALL_TILES - 1, ALL_TILES - 2, ALL_TILES, 4000, N - 3, 2047, 3071]
    lo, hi = _tensor_pair(dev, [(a, a + 3) for a in starts], B)
    idx, val = _check(ops, q, s, ops.SplitBank(s), k, lo, hi, False)
    assert bool((idx[:, :3] >= 0).all()) and bool((idx[:, 3:] == -1).all()) and bool((val[:, 3:] == NEG_INF).all())
    assert torch.equal(idx[:, :3].sort(dim=1).values, lo[:, None] + torch.arange(3, device=dev)[None, :])
    assert bool(launches) == split_always


def test_leave_one_out(dev, ops, split_always, launches):
    """The queries are bank rows; window [b, b+1) excluded: row b (the nearest: distance 0) is absent, the rest is the
    reference."""
    B, N, d, k = 130, 1000, 64, 10
    _, s = _data(dev, B, N, d)
    q = s[:B].clone()
    bank = ops.SplitBank(s)
    me = torch.arange(B, device=dev)
    assert torch.equal(ops.nw_knn(q, bank, 1, support=s)[:, 0], me)
    idx, _ = _check(ops, q, s, bank, k, me, me + 1, True)
    assert not bool((idx == me[:, None]).any())
    assert bool((idx >= 0).all())
    assert bool(launches) == split_always


# ---- every tile height, every score kind
@pytest.mark.parametrize("rs", [2, 4, 5, 6, 8, 10])
def test_every_tile_height(dev, ops, monkeypatch, rs):
    from nwhead_amd import _lib
    monkeypatch.setenv("NW_SPLIT_ALWAYS", "1")
    monkeypatch.setenv("NW_TILE_RS", str(rs))
    _lib.sync_knobs()
    try:
        from nwhead_amd.ops import _WS_BYTES
        _WS_BYTES.clear()                      # sizes answered under another tile height
        BS = 16 * rs
        B, N, d = 70, BS * 3 + 20, 64
        q, s = _data(dev, B, N, d)
        bank = ops.SplitBank(s)
        calls = _window_calls(monkeypatch)
        clo, chi = _class_windows(dev, B, N)
        pairs = [(BS, 2 * BS), (BS + 3, BS + 9), (BS - 1, BS + 1), (N - 30, N), (3 * BS, N), (0, BS), (5, 8), (BS, N)]
        plo, phi = _tensor_pair(dev, pairs, B)
        for exclude in (False, True):
            for k in (1, 7, 32):
                _check(ops, q, s, bank, k, clo, chi, exclude)
                _check(ops, q, s, bank, k, plo, phi, exclude)
        assert len(calls) == 24
    finally:
        monkeypatch.delenv("NW_TILE_RS")
        _lib.sync_knobs()
        _WS_BYTES.clear()


@pytest.mark.parametrize("kind", ["euclidean", "cosine", "dotproduct", "hypersphere_euclidean", "clip"])
def test_score_kinds(dev, ops, split_always, launches, kind):
    B, N, d = 37, 4100, 96
    q, s = _data(dev, B, N, d)
    ls = torch.tensor(2.5, device=dev) if kind == "clip" else None
    lo, hi = _class_windows(dev, B, N)
    for exclude in (False, True):
        _check(ops, q, s, ops.SplitBank(s), 10, lo, hi, exclude, kind, ls)
    assert bool(launches) == split_always


# ---- ties
def test_ties_inside_a_window(dev, ops, split_always, launches):
    """The construction of test_ties_keep_the_lowest_rows_in_order (small integers: equal rows score bit-equal in every
    tile).  The lowest admitted rows come first, in order; a tied row that the window does not admit is not returned."""
    B, N, d = 8, 2048, 64
    q, s = _data(dev, B, N, d)
    s = s.clone()
    g = torch.Generator().manual_seed(3)
    s[[100, 1919, 300]] = torch.randint(-3, 4, (3, d), generator=g).float().to(dev)
    s[101] = s[100]
    s[1920] = s[1919]
    copies = list(range(300, 300 + 40 * 11, 11))
    s[copies] = s[300].clone()
    q[0], q[1], q[2], q[3] = s[100], s[1919], s[300], s[300]
    bank = ops.SplitBank(s)
    lo = torch.tensor([101, 1919, copies[5], copies[3], 0, 0, 0, 0], device=dev)
    hi = torch.tensor([N, 1920, copies[25], copies[3] + 1, N, N, N, N], device=dev)
    idx, _ = _check(ops, q, s, bank, 32, lo, hi, False)
    assert idx[0, 0].item() == 101 and 100 not in idx[0].tolist()
    assert idx[1].tolist() == [1919] + [-1] * 31
    assert idx[2, :20].tolist() == copies[5:25] and not (set(idx[2].tolist()) & (set(copies[:5]) | set(copies[25:])))
    assert idx[3].tolist() == [copies[3]] + [-1] * 31
    idx, _ = _check(ops, q, s, bank, 32, lo, hi, True)
    assert idx[0, 0].item() == 100 and 101 not in idx[0].tolist()
    assert idx[1, 0].item() == 1920 and 1919 not in idx[1].tolist()
    assert idx[2, :20].tolist() == copies[:5] + copies[25:] and not (set(idx[2].tolist()) & set(copies[5:25]))
    assert idx[3, :32].tolist() == (copies[:3] + copies[4:])[:32]
    idx, _ = _check(ops, q, s, bank, 1, lo, hi, False)
    assert idx[:4, 0].tolist() == [101, 1919, copies[5], copies[3]]
    assert bool(launches) == split_always


# ---- a workspace that holds garbage beforehand
@pytest.mark.parametrize("exclude", [False, True], ids=["inside", "excluded"])
def test_poisoned_workspace(dev, ops, monkeypatch, exclude):
    from nwhead_amd import _lib
    monkeypatch.setenv("NW_SPLIT_ALWAYS", "1")
    B, N, d, k = 70, 2068, 64, 10
    q, s = _data(dev, B, N, d)
    bank = ops.SplitBank(s)
    lo, hi = _class_windows(dev, B, N)
    lo[:4], hi[:4] = 5, 8                       # fewer than k rows: empty slots are selected from the candidates
    calls = _window_calls(monkeypatch)
    first = ops.nw_knn(q, bank, k, return_values=True, support=s, row_window=(lo, hi), exclude=exclude)
    torch.cuda.synchronize()
    need = int(_lib.load().nw_knn_workspace_bytes(B, N, bank.shape[1], k))
    assert need > 0 and ws_poison.poison_cached_workspaces(need, dev) >= need
    again = ops.nw_knn(q, bank, k, return_values=True, support=s, row_window=(lo, hi), exclude=exclude)
    torch.cuda.synchronize()
    assert len(calls) == 2
    assert torch.equal(again[0], first[0]) and torch.equal(again[1].view(torch.int32), first[1].view(torch.int32))
    assert not bool(torch.isnan(again[1]).any())
    _check(ops, q, s, bank, k, lo, hi, exclude)


# ---- the two routes of ops.nw_knn
@pytest.mark.parametrize("exclude", [False, True], ids=["inside", "excluded"])
def test_fused_and_score_matrix_routes_agree(dev, ops, monkeypatch, exclude):
    B, N, d, k = 64, 10000, 128, 10
    q, s = _data(dev, B, N, d)
    bank = ops.SplitBank(s)
    lo, hi = _class_windows(dev, B, N, C=200)
    lo[:3], hi[:3] = 4000, 4004                 # padded lists agree too
    calls = _window_calls(monkeypatch)
    monkeypatch.setenv("NW_SPLIT_ALWAYS", "1")
    fused = ops.nw_knn(q, bank, k, return_values=True, support=s, row_window=(lo, hi), exclude=exclude)
    assert calls == [(B, N, d, k)]
    # k = 33 leaves the fused search (the tile epilogue holds 32 keys): same scores, masked by torch ops
    wide = ops.nw_knn(q, bank, 33, return_values=True, support=s, row_window=(lo, hi), exclude=exclude)
    assert len(calls) == 1
    count = _admitted(N, lo, hi, exclude).sum(1)
    assert torch.equal(wide[0][:, :k], fused[0]) and torch.equal(wide[1][:, :k], fused[1])
    assert bool(((wide[0] == -1) == (torch.arange(33, device=dev)[None, :] >= count[:, None])).all())
    assert bool(((wide[1] == NEG_INF) == (wide[0] == -1)).all())


# ---- refusals
def test_refusals(dev, ops):
    B, N, d = 4, 100, 64
    q, s = _data(dev, B, N, d)
    bank = ops.SplitBank(s)
    lo, hi = torch.zeros(B, dtype=torch.int64, device=dev), torch.full((B,), 50, device=dev)
    with pytest.raises(ops.NWHipError, match="no window form"):
        ops.nw_knn(q, ops.SplitBank(_data(dev, B, N, 192)[1], precision="fp16"), 3, rounded=True, row_window=(lo, hi))
    with pytest.raises(ValueError):
        ops.nw_knn(q, bank, 3, support=s, row_window=(lo[:3], hi))
    with pytest.raises(ValueError):
        ops.nw_knn(q, bank, 3, support=s, row_window=(lo, hi[:, None]))
    with pytest.raises(ValueError):
        ops.nw_knn(q, bank, 3, support=s, row_window=(lo.float(), hi))
    with pytest.raises(ValueError):
        ops.nw_knn(q, bank, 3, support=s, row_window=(lo, hi.bool()))
    with pytest.raises(ValueError):
        ops.nw_knn(q, bank, 3, support=s, row_window=(lo.cpu(), hi.cpu()))
    with pytest.raises(ValueError):
        ops.nw_knn(q, bank, 3, support=s, row_window=lo)
    for k in (0, N + 1):
        with pytest.raises(ops.NWHipError):
            ops.nw_knn(q, bank, k, support=s, row_window=(lo, hi))
    idx = ops.nw_knn(q, bank, 3, support=s, row_window=(lo.int(), hi.int()))       # int32 is taken as it is
    assert idx.shape == (B, 3) and int(idx.max()) < 50
