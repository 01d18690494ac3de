"""ops.nw_head(..., support_cache=bank, row_window=(lo, hi), exclude=...) / nw_fwd_window_f32: the head of every query over
its own row window of a prepared bank, kept or excluded, without the (B,N) score matrix -- the epilogue of the split-fp16
tile kernel turns the scores of the rows a window does not admit into -inf BEFORE the tile maximum (fused_impl.h, OUT_WIN), a
(query, tile) pair that keeps no row stores m = -inf, den = 0 and zero run sums, and the run merge gives a query without
any row log(1e-12) everywhere and lse = -inf.

Reference: the head in fp64 from the fp32 inputs with the mask applied to the fp64 score matrix (scores -> -inf -> softmax
-> one-hot product -> log(. + 1e-12)).  Tolerance: the bank-path bound of test_hip_parity.py, rtol 1e-5 and atol
max(3e-5, 3e-6 * max|score|); its floor for the -27.63 "absent class" entries is what rtol gives them (2.8e-4).  Every
comparison runs on a workspace filled with 0xFF beforehand (ws_poison) and asserts finite outputs."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ws_poison
from test_knn_fused_gpu import _data, dev, ops  # noqa: F401  (fixtures and the generator, by import)

pytestmark = pytest.mark.gpu

NEG_INF = float("-inf")
LOG_EPS = math.log(1e-12)
ALL_TILES = 1920          # a multiple of every tile height
KINDS = ("euclidean", "hypersphere_euclidean", "cosine", "dotproduct", "clip")
SHAPES = [(37, 4100, 96), (130, 1000, 64), (256, 2048, 512)]


@pytest.fixture(autouse=True)
def _no_split_always(monkeypatch):
    monkeypatch.delenv("NW_SPLIT_ALWAYS", raising=False)     # the windowed head is fused without it


def _spy(monkeypatch):
    """Records the (B, N, d, C) of every nw_fwd_window_f32 launch: which route a call took."""
    from nwhead_amd import _lib
    lib = _lib.load()
    real = lib.nw_fwd_window_f32
    calls = []

    class Spy:
        def __getattr__(self, name):
            if name == "nw_fwd_window_f32":
                return lambda *a: (calls.append(a[12:16]), real(*a))[1]
            return getattr(lib, name)

    monkeypatch.setattr(_lib, "_lib", Spy())
    return calls


@pytest.fixture
def launches(monkeypatch):
    return _spy(monkeypatch)


def _scores_f64(q, s, kind, ls=None):
    q, s = q.double(), s.double()
    if kind in ("hypersphere_euclidean", "cosine", "clip"):
        q = q / q.norm(dim=-1, keepdim=True).clamp_min(1e-12)
        s = s / s.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    if kind in ("euclidean", "hypersphere_euclidean"):
        return -torch.cdist(q, s, compute_mode="donot_use_mm_for_euclid_dist")
    dot = q @ s.T
    return math.exp(float(ls)) * dot if kind == "clip" else dot


def _admitted(N, lo, hi, exclude):
    cols = torch.arange(N, device=lo.device)
    inside = (cols >= lo[:, None]) & (cols < hi[:, None])
    return ~inside if exclude else inside


def _reference(q, s, sy, C, lo, hi, exclude, kind="euclidean", ls=None):
    """-> (log-probs fp64, lse fp64, max |score|)."""
    sc = _scores_f64(q, s, kind, ls)
    masked = sc.masked_fill(~_admitted(s.shape[0], lo, hi, exclude), NEG_INF)
    w = torch.softmax(masked, dim=-1)
    w = torch.where(torch.isnan(w), torch.zeros_like(w), w)             # a window without a row: no weight anywhere
    out = torch.log(w @ F.one_hot(sy, C).double() + 1e-12)
    return out, torch.logsumexp(masked, dim=-1), sc.abs().max().item()


def _close(got, ref, smax):
    assert bool(torch.isfinite(got).all())
    np.testing.assert_allclose(got.cpu().double().numpy(), ref.cpu().numpy(), rtol=1e-5, atol=max(3e-5, 3e-6 * smax))


def _head(ops, q, s, sy, C, bank, lo, hi, exclude, kind="euclidean", ls=None, lse=False):
    """The windowed head on a poisoned workspace."""
    need = ws_poison.fwd_workspace_bytes(q.shape[0], s.shape[0], bank.shape[1], C)
    torch.cuda.synchronize()
    assert need > 0 and ws_poison.poison_cached_workspaces(need, q.device) >= need
    if lse:
        return ops.nw_head_window(q, s, sy, C, bank, (lo, hi), exclude, kind, ls, return_lse=True)
    return ops.nw_head(q, s, sy, C, kind, ls, support_cache=bank, row_window=(lo, hi), exclude=exclude)


def _check(ops, q, s, sy, C, bank, lo, hi, exclude, kind="euclidean", ls=None):
    out = _head(ops, q, s, sy, C, bank, lo, hi, exclude, kind, ls)
    ref, _, smax = _reference(q, s, sy, C, lo, hi, exclude, kind, ls)
    assert out.shape == (q.shape[0], C) and out.dtype == torch.float32
    _close(out, ref, smax)
    return out


def _sorted_labels(dev, N, C=16):
    return (torch.arange(N) % C).sort().values.to(dev)


def _class_windows(dev, sy, B, C=16, seed=11):
    qy = torch.randint(0, C, (B,), generator=torch.Generator().manual_seed(seed)).to(dev)
    return torch.searchsorted(sy, qy), torch.searchsorted(sy, qy, right=True)


def _tensor_pair(dev, pairs, B):
    lo = torch.tensor([pairs[b % len(pairs)][0] for b in range(B)], device=dev)
    hi = torch.tensor([pairs[b % len(pairs)][1] for b in range(B)], device=dev)
    return lo, hi


# ---- 1. class windows
@pytest.mark.parametrize("exclude", [False, True], ids=["kept", "excluded"])
@pytest.mark.parametrize("B,N,d", SHAPES)
def test_class_windows(dev, ops, launches, B, N, d, exclude):
    C = 16
    q, s = _data(dev, B, N, d)
    sy = _sorted_labels(dev, N, C)
    lo, hi = _class_windows(dev, sy, B, C)
    out = _check(ops, q, s, sy, C, ops.SplitBank(s, labels=sy), lo, hi, exclude)
    assert launches == [(B, N, d, C)], "fused at every shape the kernel takes, without NW_SPLIT_ALWAYS"
    qy = sy[lo]
    mine = out[torch.arange(B, device=dev), qy]
    if exclude:       # the query's class is absent
        assert bool(((mine - LOG_EPS).abs() < 3e-4).all())
    else:             # and here it is the only one
        assert bool((mine.abs() < 1e-5).all()) and bool(((out.sum(1) - mine - (C - 1) * LOG_EPS).abs() < 1e-2).all())


@pytest.mark.parametrize("kind", KINDS)
def test_score_kinds(dev, ops, launches, kind):
    B, N, d, C = 37, 4100, 96, 16
    q, s = _data(dev, B, N, d)
    sy = _sorted_labels(dev, N, C)
    ls = torch.tensor(2.5, device=dev) if kind == "clip" else None
    lo, hi = _class_windows(dev, sy, B, C)
    bank = ops.SplitBank(s, labels=sy)
    for exclude in (False, True):
        _check(ops, q, s, sy, C, bank, lo, hi, exclude, kind, ls)
    assert len(launches) == 2


# ---- 2. tile boundaries
@pytest.mark.parametrize("exclude", [False, True], ids=["kept", "excluded"])
def test_windows_at_tile_boundaries(dev, ops, launches, exclude):
    """The windows of test_knn_window_gpu.py's test of the same name: strictly inside one tile, on boundaries of every
    height, the ragged last tile, one row either side of a boundary, single rows, the first and the last row."""
    B, N, d, C = 37, 4100, 96, 16
    q, s = _data(dev, B, N, d)
    sy = _sorted_labels(dev, N, C)
    pairs = [(ALL_TILES + 5, ALL_TILES + 20), (ALL_TILES, 2 * ALL_TILES), (4000, N), (4097, N), (ALL_TILES - 1, ALL_TILES + 1),
             (0, ALL_TILES), (ALL_TILES, N), (2000, 2001), (0, 1), (N - 1, N), (ALL_TILES - 40, ALL_TILES)]
    lo, hi = _tensor_pair(dev, pairs, B)
    _check(ops, q, s, sy, C, ops.SplitBank(s, labels=sy), lo, hi, exclude)
    assert len(launches) == 1


@pytest.mark.parametrize("rs", [2, 4, 5, 6, 8, 10])
def test_every_tile_height(dev, ops, monkeypatch, rs):
    from nwhead_amd import _lib
    monkeypatch.setenv("NW_TILE_RS", str(rs))
    _lib.sync_knobs()
    try:
        from nwhead_amd.ops import _WS_BYTES
        _WS_BYTES.clear()                      # sizes answered under another tile height
        BS = 16 * rs
        B, N, d, C = 70, BS * 3 + 20, 64, 16
        q, s = _data(dev, B, N, d)
        sy = _sorted_labels(dev, N, C)
        bank = ops.SplitBank(s, labels=sy)
        calls = _spy(monkeypatch)
        clo, chi = _class_windows(dev, sy, B, C)
        pairs = [(BS, 2 * BS), (BS + 3, BS + 9), (BS - 1, BS + 1), (N - 30, N), (3 * BS, N), (0, BS), (5, 8), (BS, N),
                 (0, 1), (N - 1, N), (2 * BS, 2 * BS + 1), (2 * BS - 1, 2 * BS)]
        plo, phi = _tensor_pair(dev, pairs, B)
        for exclude in (False, True):
            _check(ops, q, s, sy, C, bank, clo, chi, exclude)
            _check(ops, q, s, sy, C, bank, plo, phi, exclude)
        assert len(calls) == 4
    finally:
        monkeypatch.delenv("NW_TILE_RS")
        _lib.sync_knobs()
        _WS_BYTES.clear()


# ---- 3. degenerate windows
def test_degenerate_windows(dev, ops, launches):
    B, N, d, C = 37, 4100, 96, 16
    q, s = _data(dev, B, N, d)
    sy = _sorted_labels(dev, N, C)
    bank = ops.SplitBank(s, labels=sy)
    plain = ops.nw_head(q, s, sy, C, support_cache=bank)
    at = torch.full((B,), 777, device=dev)
    zero, full = torch.zeros(B, dtype=torch.int64, device=dev), torch.full((B,), N, device=dev)
    smax = _scores_f64(q, s, "euclidean").abs().max().item()

    def nothing(lo, hi, exclude):
        out, lse = _head(ops, q, s, sy, C, bank, lo, hi, exclude, lse=True)
        assert bool(torch.isfinite(out).all()) and not bool(torch.isnan(lse).any())
        assert bool(((out - LOG_EPS).abs() < 1e-5 * abs(LOG_EPS)).all()) and bool((lse == NEG_INF).all())
        _close(out, _reference(q, s, sy, C, lo, hi, exclude)[0], smax)

    def everything(lo, hi, exclude):
        out, lse = _head(ops, q, s, sy, C, bank, lo, hi, exclude, lse=True)
        _close(out, plain.double(), smax)
        ref, ref_lse, _ = _reference(q, s, sy, C, lo, hi, exclude)
        _close(out, ref, smax)
        _close(lse, ref_lse, smax)

    nothing(at, at, False)                      # lo == hi
    everything(at, at, True)
    nothing(at, at - 100, False)                # lo > hi is empty too
    everything(at, at - 100, True)
    everything(zero, full, False)               # the whole bank
    nothing(zero, full, True)
    everything(zero - 5, full + (1 << 30), False)   # clamped, never used as an address
    nothing(zero - 5, full + (1 << 30), True)
    nothing(zero - 9, zero - 5, False)          # wholly outside the bank, either side
    nothing(full + 5, full + 9, False)
    # half the queries without a row, the others with a class window
    lo, hi = _class_windows(dev, sy, B, C)
    lo[::2], hi[::2] = 900, 900
    out, lse = _head(ops, q, s, sy, C, bank, lo, hi, False, lse=True)
    ref, ref_lse, _ = _reference(q, s, sy, C, lo, hi, False)
    _close(out, ref, smax)
    assert bool((lse[::2] == NEG_INF).all())
    _close(lse[1::2], ref_lse[1::2], smax)
    assert len(launches) == 11


# ---- 4. leave-one-out where subtracting the self term fails
def test_leave_one_out_far_neighbours(dev, ops, launches):
    """Queries are bank rows whose nearest other row is farther than 20: in fp32 the full softmax is the self term alone
    (den == 1.0 exactly), so no arithmetic on its outputs can recover the leave-one-out head.  Classes sit around centres 40
    apart (spread 1 per coordinate in 512 dimensions: rows of a class ~32 apart, of two classes ~51).  The last row is the
    only member of its class: left out, its true class is absent."""
    N, d, C = 1000, 512, 16
    g = torch.Generator().manual_seed(41)
    sy = (torch.arange(N - 1) % (C - 1)).sort().values
    sy = torch.cat([sy, torch.tensor([C - 1])]).to(dev)
    centres = torch.zeros(C, d)
    centres[torch.arange(C), torch.arange(C)] = 40.0 / math.sqrt(2.0)
    s = (centres[sy.cpu()] + torch.randn(N, d, generator=g)).to(dev)
    rows = torch.cat([torch.arange(0, N - 1, 8), torch.tensor([N - 1])]).to(dev)      # 126 rows, every class
    q = s[rows].clone()
    B = len(rows)
    bank = ops.SplitBank(s, labels=sy)
    other = _scores_f64(q, s, "euclidean").masked_fill(_admitted(N, rows, rows + 1, False), NEG_INF)
    assert other.max().item() < -20.0
    packed = ops.nw_partials(q, s, sy, C, support_cache=bank).view(-1)
    assert bool((packed[B:2 * B] == 1.0).all()), "vacuous otherwise: the full-bank denominator must hide every other row"
    out = _check(ops, q, s, sy, C, bank, rows, rows + 1, True)
    assert launches == [(B, N, d, C)]
    assert abs(out[-1, C - 1].item() - LOG_EPS) < 3e-4                     # no other member of its class
    assert bool((out[:-1].argmax(1) == sy[rows[:-1]]).all())               # the others find their class without themselves


# ---- 5. independence and determinism
def test_rows_do_not_depend_on_each_other(dev, ops, launches):
    B, N, d, C = 130, 1000, 64, 16
    q, s = _data(dev, B, N, d)
    sy = _sorted_labels(dev, N, C)
    bank = ops.SplitBank(s, labels=sy)
    lo, hi = _class_windows(dev, sy, B, C)
    lo[5], hi[5] = 300, 300                       # an empty one, a single row, the whole bank
    lo[70], hi[70] = 999, 1000
    lo[129], hi[129] = 0, N
    for exclude in (False, True):
        mixed = _head(ops, q, s, sy, C, bank, lo, hi, exclude)
        assert torch.equal(_head(ops, q, s, sy, C, bank, lo, hi, exclude), mixed)
        for b in (0, 5, 63, 64, 70, 129):
            same = _head(ops, q, s, sy, C, bank, lo[b].expand(B).contiguous(), hi[b].expand(B).contiguous(), exclude)
            assert torch.equal(same[b], mixed[b])
        perm = torch.randperm(B, generator=torch.Generator().manual_seed(2)).to(dev)
        shuffled = _head(ops, q[perm].contiguous(), s, sy, C, bank, lo[perm], hi[perm], exclude)
        assert torch.equal(shuffled, mixed[perm])
    assert len(launches) == 2 * (2 + 6 + 1)


# ---- 6. a dead tile between live ones
@pytest.mark.parametrize("rs", [4, 8])
def test_dead_tile_between_live_ones(dev, ops, monkeypatch, rs):
    """Three tiles; the excluded window is exactly the middle one.  Every query (whole waves skip the tile), every other
    query (dead columns next to live ones in a wave), and a kept window that leaves only the middle tile alive."""
    from nwhead_amd import _lib
    monkeypatch.setenv("NW_TILE_RS", str(rs))
    _lib.sync_knobs()
    try:
        from nwhead_amd.ops import _WS_BYTES
        _WS_BYTES.clear()
        BS = 16 * rs
        B, N, d, C = 70, 2 * BS + 50, 64, 16
        q, s = _data(dev, B, N, d)
        sy = _sorted_labels(dev, N, C)
        bank = ops.SplitBank(s, labels=sy)
        calls = _spy(monkeypatch)
        lo, hi = torch.full((B,), BS, device=dev), torch.full((B,), 2 * BS, device=dev)
        _check(ops, q, s, sy, C, bank, lo, hi, True)
        _check(ops, q, s, sy, C, bank, lo, hi, False)
        lo2, hi2 = lo.clone(), hi.clone()
        lo2[::2], hi2[::2] = 0, 0
        _check(ops, q, s, sy, C, bank, lo2, hi2, True)
        lo2[::2], hi2[::2] = 0, N
        _check(ops, q, s, sy, C, bank, lo2, hi2, False)
        assert len(calls) == 4
    finally:
        monkeypatch.delenv("NW_TILE_RS")
        _lib.sync_knobs()
        _WS_BYTES.clear()


# ---- 7. NWNet
def _net(dev, ops, **kw):
    from nwhead_amd.nwhead.nw import NWNet

    class DS(torch.utils.data.Dataset):
        def __init__(self):
            g = torch.Generator().manual_seed(5)
            self.x = torch.randn(400, 48, generator=g)
            self.targets = (torch.arange(400) // 40).tolist()

        def __len__(self):
            return 400

        def __getitem__(self, i):
            return self.x[i], self.targets[i]

    torch.manual_seed(0)
    net = NWNet(torch.nn.Linear(48, 64), 10, support_dataset=DS(), n_shot_full=40, device=dev, **kw).to(dev).eval()
    with torch.no_grad():
        net.precompute()
    return net


def test_nwnet_leave_out_and_predict_loo(dev, ops, launches):
    net = _net(dev, ops)
    N, C = net.full_feat.shape[0], 10
    with torch.no_grad():
        x = torch.randn(9, 48, generator=torch.Generator().manual_seed(6)).to(dev)
        qf = net._eval_featurizer()(x)
        rows = torch.tensor([3, -1, 399, 0, -1, 17, 200, 201, 40], device=dev)
        lo = rows.clamp(min=0)
        hi = torch.where(rows < 0, lo, lo + 1)
        for labelled in (True, False):     # precompute()'s bank, and a bank of the rows as they stand (always fused)
            if not labelled:
                net.full_cache = ops.SplitBank(net.full_feat)
            n0 = len(launches)
            out = net.predict(x, 'full', leave_out=rows)
            ref, _, smax = _reference(qf, net.full_feat, net.full_y, C, lo, hi, True)
            _close(out, ref, smax)
            plain = net.predict(x, 'full')
            none = rows < 0
            _close(out[none], plain[none].double(), smax)
            fused = net.full_cache.sorted_rows is None
            assert len(launches) - n0 == (1 if fused else 0)
            assert fused or labelled
            # predict_loo: every bank row without itself == leave_out row by row
            loo = net.predict_loo(batch_size=128)
            assert loo.shape == (N, C)
            me = torch.arange(N, device=dev)
            ref, _, smax = _reference(net.full_feat, net.full_feat, net.full_y, C, me, me + 1, True)
            _close(loo, ref, smax)
            some = torch.tensor([7, 399, 128, 0], device=dev)
            by_row = ops.nw_head(net.full_feat[some], net.full_feat, net.full_y, C, support_cache=net.full_cache,
                                 row_window=(some, some + 1), exclude=True)
            assert torch.equal(net.predict_loo(some), by_row)
            _close(by_row, loo[some].double(), smax)
        net.return_mask = True
        out, mask = net.predict(x, 'full', leave_out=rows)
        assert out.shape == (9, C) and mask.shape == (9,) and bool(mask.all())
        out, mask = net.predict_loo(some)
        assert out.shape == (4, C) and mask.shape == (4,)
        net.return_mask = False
        # refusals
        for mode in ('random', 'knn', 'ensemble', 'cluster'):
            with pytest.raises(ops.NWHipError, match="only mode='full'"):
                net.predict(x, mode, leave_out=rows)
        with pytest.raises(ValueError):
            net.predict(x, 'full', leave_out=rows[:4])
        net.sharded_bank = object()                       # what precompute_sharded() leaves behind
        with pytest.raises(ops.NWHipError, match="sharded"):
            net.predict(x, 'full', leave_out=rows)
        with pytest.raises(ops.NWHipError, match="sharded"):
            net.predict_loo()
        net.sharded_bank = None


# ---- 8. the score-matrix route
def test_fallback_route_agrees(dev, ops, launches):
    B, N, d, C = 37, 4100, 192, 16
    q, s = _data(dev, B, N, d)
    sy = _sorted_labels(dev, N, C)
    lo, hi = _class_windows(dev, sy, B, C)
    lo[3], hi[3] = 50, 50
    ref_bank = ops.SplitBank(s, labels=sy)
    g = torch.Generator().manual_seed(1)
    perm = torch.randperm(N, generator=g).to(dev)
    for exclude in (False, True):
        fused = _check(ops, q, s, sy, C, ref_bank, lo, hi, exclude)
        n0 = len(launches)
        half = ops.SplitBank(s, labels=sy, precision="fp16")
        assert half.split is None
        out, lse = _head(ops, q, s, sy, C, half, lo, hi, exclude, lse=True)
        ref, ref_lse, smax = _reference(q, s, sy, C, lo, hi, exclude)
        _close(out, ref, smax)
        _close(out, fused.double(), smax)
        empty = ~_admitted(N, lo, hi, exclude).any(1)
        assert bool((lse[empty] == NEG_INF).all())
        _close(lse[~empty], ref_lse[~empty], smax)
        # unsorted labels: the bank holds a class-sorted copy, the windows are rows of the caller's tensor
        s2, sy2 = s[perm].contiguous(), sy[perm].contiguous()
        unsorted = ops.SplitBank(s2, labels=sy2)
        assert unsorted.sorted_rows is not None
        out = _head(ops, q, s2, sy2, C, unsorted, lo, hi, exclude)
        ref, _, smax = _reference(q, s2, sy2, C, lo, hi, exclude)
        _close(out, ref, smax)
        # N <= 25: no tile kernel takes it
        s20, sy20 = s[:20].contiguous(), (torch.arange(20, device=dev) % C).contiguous()
        tiny = ops.SplitBank(s20)
        tlo = lo % 20
        thi = (tlo + hi % 7).clamp(max=20)            # some of them empty
        out = _head(ops, q, s20, sy20, C, tiny, tlo, thi, exclude)
        ref, _, smax = _reference(q, s20, sy20, C, tlo, thi, exclude)
        _close(out, ref, smax)
        assert len(launches) == n0, "none of these banks is served by the fused kernel"
