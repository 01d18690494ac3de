"""The neighbour search over the half-precision bank (nw_knn_f16, ops.nw_knn(rounded=True), NWNet / ShardedBank with
search_precision="fp16"): the candidate form of the persistent 256-query kernel.

Reference: S = the fp64 scores (oracle.nw_oracle.scores_f64) of the ROUNDED queries against the ROUNDED rows (the rounding of
nw_pack_rows_f16, restated by test_half_bank_gpu._round_rows).  The kernel's scores lie within
    tol(x) = max(3e-5, 3e-6 max|S|) + 1e-5 |x|
of S (the bound of test_half_bank_gpu.py for this kernel on rounded operands: its _atol and RTOL), so for every query, with T
the k-th largest S of that query, an exact top-k of such scores satisfies (_check):
  * rows distinct and inside [0, N); values non-increasing, bit-equal values in ascending row order;
  * |val - S[row]| <= tol(S[row]);
  * S[row] >= T - (tol(S[row]) + t_top), t_top = the largest tol over the true top k: the k-th returned score is at least the
    k-th largest computed one, which is at least min over the true top k of S - tol;
  * every row j with S[j] > T + tol(S[j]) + t_ret is returned, t_ret = the largest tol over the returned rows: at least one
    returned row has S <= T, and a row left out scores no more than it.
Both margins are "2 tol" with each tol taken where it arises.  No query is excluded.  A query whose top-(k+1)
consecutive fp64 gaps all exceed twice the larger tol of the two neighbours is "clear": its rows must equal the fp64 top-k.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import ws_poison
from test_half_bank_gpu import RTOL, _DS, _inputs, _ls, _round_rows

pytestmark = pytest.mark.gpu

KINDS = ("euclidean", "hypersphere_euclidean", "cosine", "dotproduct", "clip")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "run with -m gpu on the MI355X box"
    from nwhead_amd import _lib
    _lib.check(_lib.load().nw_device_check(), "nw_device_check")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from nwhead_amd import ops as o
    return o


@pytest.fixture(scope="module")
def O():
    from oracle import nw_oracle
    return nw_oracle


def _scores64(O, q, s, kind):
    """fp64 scores of the rounded operands, on the device, 64 queries at a time."""
    q_r, s_r = _round_rows(q)[3], _round_rows(s)[3]
    return torch.cat([O.scores_f64(q_r[a:a + 64], s_r, kind, O.CLIP_LOGIT_SCALE_INIT) for a in range(0, len(q_r), 64)])


@functools.lru_cache(maxsize=None)
def _case(B, N, d, kind):
    """(q, s, S) of one shape and score kind: the generator of test_half_bank_gpu._inputs (seed 0), S computed once and
    shared by the tests that need it (nobody writes to it)."""
    from oracle import nw_oracle
    q, s, _ = _inputs(B, N, d, torch.device("cuda:0"))
    return q, s, _scores64(nw_oracle, q, s, kind)


def _tol_fn(S):
    floor = max(3e-5, 3e-6 * S.abs().max().item())
    return lambda x: floor + RTOL * x.abs()


def _check(idx, val, S, k):
    """The conditions of the module docstring, for every query; returns the tolerance function."""
    B, N = S.shape
    tol = _tol_fn(S)
    assert idx.shape == (B, k) and idx.dtype == torch.int64 and val.shape == (B, k) and val.dtype == torch.float32
    assert int(idx.min()) >= 0 and int(idx.max()) < N
    srt = torch.sort(idx, dim=1).values
    assert bool((srt[:, 1:] != srt[:, :-1]).all()), "rows are distinct"
    assert bool((val[:, 1:] <= val[:, :-1]).all()), "values are non-increasing"
    same = val[:, 1:].view(torch.int32) == val[:, :-1].view(torch.int32)
    assert bool((idx[:, 1:] > idx[:, :-1])[same].all()), "bit-equal values come in ascending row order"
    got = torch.gather(S, 1, idx)
    err = (val.double() - got).abs()
    print(f"max |val - S| / tol = {(err / tol(got)).max().item():.3f}")
    assert bool((err <= tol(got)).all()), (err / tol(got)).max().item()
    top = torch.topk(S, k, dim=1).values
    T = top[:, k - 1:k]
    t_top = tol(top).max(dim=1, keepdim=True).values
    assert bool((got >= T - (tol(got) + t_top)).all()), "a returned row is further than the k-th best by more than the bound"
    t_ret = tol(got).max(dim=1, keepdim=True).values
    must = S > T + tol(S) + t_ret
    returned = torch.zeros_like(must).scatter_(1, idx, True)
    assert bool((returned | ~must).all()), "a row clearly better than the k-th best is missing"
    return tol


def _clear(S, k, tol):
    """Queries whose top-(k+1) consecutive fp64 gaps all exceed twice the tolerance (the larger of the two neighbours')."""
    top = torch.topk(S, min(k + 1, S.shape[1]), dim=1).values
    gaps = top[:, :-1] - top[:, 1:]
    return (gaps > 2 * torch.maximum(tol(top[:, :-1]), tol(top[:, 1:]))).all(dim=1)


def _search(ops, q, s, k, kind, dev, **kw):
    bank = ops.SplitBank(s, precision="fp16")
    assert bank.packed is not None and bank.sorted_rows is None
    idx, val = ops.nw_knn(q, bank, k, kind, _ls(kind, dev), return_values=True, rounded=True, **kw)
    torch.cuda.synchronize()
    return idx, val


# (B, N, d), k, kinds: one ragged tile, k = N; a second query tile with one live row and a last support tile with one row
# (nine of its ten slots stay empty); 9 support tiles, 3 stages, every kind; 7 stages
CASES = [((1, 26, 192), 1, ("euclidean",)), ((1, 26, 192), 26, ("euclidean",)), ((257, 129, 256), 10, ("euclidean",)),
         ((300, 1100, 192), 1, KINDS), ((300, 1100, 192), 10, KINDS), ((300, 1100, 192), 32, KINDS),
         ((64, 640, 448), 32, ("euclidean",))]
CASES = [(shape, k, kind) for shape, k, kinds in CASES for kind in kinds]


@pytest.mark.parametrize("shape,k,kind", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_conditions_against_fp64_on_rounded_operands(dev, ops, shape, k, kind):
    q, s, S = _case(*shape, kind)
    idx, val = _search(ops, q, s, k, kind, dev)
    _check(idx, val, S, k)


def test_many_tiles_per_workgroup(dev, ops):
    """82 support tiles x 2 query tiles on 8 workgroups (nw_fwd_opts.persistent_wgs): every workgroup walks about ten tiles."""
    q, s, S = _case(300, 5125, 192, "euclidean")
    idx, val = _search(ops, q, s, 10, "euclidean", dev, persistent_wgs=8)
    tol = _check(idx, val, S, 10)
    clear = _clear(S, 10, tol)
    print(f"clear queries: {clear.float().mean().item():.3f}")
    assert clear.float().mean().item() >= 0.85, "vacuous"
    assert torch.equal(idx[clear], torch.topk(S, 10, dim=1).indices[clear])


@pytest.mark.parametrize("k", [1, 10])
@pytest.mark.parametrize("kind", ["euclidean", "dotproduct", "clip"])
def test_rows_of_clear_queries_equal_the_fp64_top_k(dev, ops, kind, k):
    q, s, S = _case(300, 1100, 192, kind)
    idx, val = _search(ops, q, s, k, kind, dev)
    clear = _clear(S, k, _tol_fn(S))
    print(f"clear queries: {clear.float().mean().item():.3f}")
    assert clear.float().mean().item() >= 0.85, "vacuous"
    assert torch.equal(idx[clear], torch.topk(S, k, dim=1).indices[clear])


@pytest.mark.parametrize("d,padded", [(64, 192), (200, 256)])
def test_padded_widths(dev, ops, O, d, padded):
    B, N, k = 70, 300, 10
    q, s, _ = _inputs(B, N, d, dev, seed=9)
    bank = ops.SplitBank(s, precision="fp16")
    assert bank.pad == padded - d and bank.packed.shape == (N, padded)
    idx, val = ops.nw_knn(q, bank, k, return_values=True, rounded=True)       # queries of the caller's width
    torch.cuda.synchronize()
    _check(idx, val, _scores64(O, q, s, "euclidean"), k)     # zero columns change neither the row maxima nor any product
    with pytest.raises(ops.NWHipError, match="width"):
        ops.nw_knn(q[:, :d - 4].contiguous(), bank, k, rounded=True)


def test_schedule_independence_and_repeatability(dev, ops):
    q, s, _ = _case(300, 5125, 192, "euclidean")
    bank = ops.SplitBank(s, precision="fp16")
    res = [ops.nw_knn(q, bank, 10, return_values=True, rounded=True, persistent_wgs=w) for w in (8, 64, 0, 0)]
    torch.cuda.synchronize()
    for idx, val in res[1:]:
        assert torch.equal(idx, res[0][0]) and torch.equal(val.view(torch.int32), res[0][1].view(torch.int32))


@pytest.mark.parametrize("shape", [(257, 129, 256), (300, 1100, 192)], ids=lambda s: "x".join(map(str, s)))
def test_poisoned_workspace(dev, ops, shape):
    from nwhead_amd import _lib
    B, N, d = shape
    q, s, _ = _case(B, N, d, "euclidean")
    bank = ops.SplitBank(s, precision="fp16")
    first = ops.nw_knn(q, bank, 10, return_values=True, rounded=True)
    torch.cuda.synchronize()
    need = int(_lib.load().nw_knn_f16_workspace_bytes(B, N, d, 10))
    assert need > 0 and ws_poison.poison_cached_workspaces(need, dev) >= need
    again = ops.nw_knn(q, bank, 10, return_values=True, rounded=True)
    torch.cuda.synchronize()
    assert torch.equal(again[0], first[0]) and torch.equal(again[1].view(torch.int32), first[1].view(torch.int32))
    assert torch.isfinite(again[1]).all()


@pytest.mark.parametrize("kind", ["euclidean", "dotproduct"])
def test_ties(dev, ops, O, kind):
    """Rows 5, 6, 7 and 200, 201 are copies of each other, each group inside one 128-row tile: for the queries nearest to
    them the copies come back with bit-equal values in ascending row order.  Row 900, a copy of row 200 in another tile, is
    held to the tolerance conditions only (the kernel rotates its k chunks by the support tile)."""
    B, N, d, k = 8, 1100, 192, 4
    q, s, g = _inputs(B, N, d, dev, seed=21)
    s[6] = s[5]
    s[7] = s[5]
    s[201] = s[200]
    s[900] = s[200]
    # the largest product with / the smallest distance to its own group.  Not the row itself: a distance near zero is the
    # root of a cancelled difference and misses every absolute bound (the other rows lie ~17 away, the group ~2.8)
    near = 0.2 * torch.randn(2, d, generator=g).to(dev)
    q[0], q[1] = (3.0 * s[5], 3.0 * s[200]) if kind == "dotproduct" else (s[5] + near[0], s[200] + near[1])
    idx, val = _search(ops, q, s, k, kind, dev)
    _check(idx, val, _scores64(O, q, s, kind), k)
    bits = val.view(torch.int32)
    assert idx[0, :3].tolist() == [5, 6, 7] and int(bits[0, 0]) == int(bits[0, 1]) == int(bits[0, 2])
    assert sorted(idx[1, :3].tolist()) == [200, 201, 900]
    p200, p201 = idx[1].tolist().index(200), idx[1].tolist().index(201)
    assert p201 == p200 + 1 and int(bits[1, p200]) == int(bits[1, p201])


def test_refusals(dev, ops):
    from nwhead_amd import _lib
    lib = _lib.load()
    q, s, _ = _inputs(8, 300, 192, dev, seed=2)
    with pytest.raises(ops.NWHipError, match="fp16"):
        ops.nw_knn(q, ops.SplitBank(s), 5, rounded=True)                                   # a split-row bank
    unsorted = (torch.arange(300, device=dev) % 7)
    with pytest.raises(ops.NWHipError, match="sorted"):
        ops.nw_knn(q, ops.SplitBank(s, labels=unsorted, precision="fp16"), 5, rounded=True)
    with pytest.raises(ops.NWHipError, match="norms-only"):
        ops.nw_knn(q, ops.SplitBank(s[:20].contiguous(), precision="fp16"), 5, rounded=True)
    bank = ops.SplitBank(s, precision="fp16")
    with pytest.raises(ops.NWHipError, match="32"):
        ops.nw_knn(q, bank, 33, rounded=True)
    # the C entry: d = 100 (no half form) and a short workspace, both before anything is launched
    idx = torch.full((8, 5), -7, dtype=torch.int64, device=dev)
    need = int(lib.nw_knn_f16_workspace_bytes(8, 300, 192, 5))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream().cuda_stream

    def call(d, ws_bytes):
        return lib.nw_knn_f16(q.data_ptr(), bank.packed.data_ptr(), bank.packed_scale.data_ptr(), bank.packed_norm2.data_ptr(),
                              idx.data_ptr(), None, ws.data_ptr(), ws_bytes, 8, 300, d, 5, 0, None, None, st)

    assert lib.nw_knn_f16_workspace_bytes(8, 300, 100, 5) == 0
    assert call(100, need) == -2 and call(192, need - 1) == -3
    torch.cuda.synchronize()
    assert bool((idx == -7).all()), "nothing was written"
    assert call(192, need) == 0
    torch.cuda.synchronize()
    assert torch.equal(idx, ops.nw_knn(q, bank, 5, rounded=True))


def test_default_is_untouched(dev, ops):
    q, s, _ = _inputs(33, 1000, 192, dev, seed=4)
    bank = ops.SplitBank(s, precision="fp16")
    idx, val = ops.nw_knn(q, bank, 10, return_values=True, support=s)
    ref_idx, ref_val = ops.nw_topk(ops.nw_scores(q, s), 10, return_values=True)
    assert torch.equal(idx, ref_idx) and torch.equal(val.view(torch.int32), ref_val.view(torch.int32))


# ------------------------------------------------------------------------------------------------------------------ NWNet
def _net(**kw):
    import torch.nn as nn
    from conftest import T, load_golden
    from nwhead_amd.nwhead.nw import NWNet
    g = load_golden("g5_nwnet_plumbing.npz")
    n_classes = int(g["C"])
    ds = _DS(T(g["ds_data"]), g["ds_targets"].tolist(), n_classes)
    feat = nn.Sequential(nn.Flatten(), nn.Linear(48, 16))
    with torch.no_grad():
        feat[1].weight.copy_(T(g["w"]))
        feat[1].bias.copy_(T(g["b"]))
    net = NWNet(feat, n_classes, support_dataset=ds, feat_dim=16, n_shot=2, n_way=6, n_shot_full=7, n_shot_cluster=2,
                n_neighbors=3, device="cuda:0", cluster_backend="sklearn", **kw).to("cuda:0")
    net.eval()
    np.random.seed(1234)
    net.precompute()
    return net, T(g["xq"]).cuda(), n_classes


def test_nwnet_search_precision_fp16(dev, ops, O, monkeypatch):
    net, xq, n_classes = _net(full_precision="fp16", search_precision="fp16", knn_per_query=True)
    bank = net.full_cache
    N = bank.shape[0]
    assert N > 25 and bank.packed is not None and bank.sorted_rows is None
    calls = []
    orig = ops.nw_knn
    monkeypatch.setattr(ops, "nw_knn", lambda *a, **kw: (calls.append(kw.get("rounded", False)), orig(*a, **kw))[1])
    with torch.no_grad():
        qfeat = net.featurizer(xq)
        idx, val = orig(qfeat, bank, 5, return_values=True, rounded=True)
        nb = net.get_neighbors(xq, 5)
        assert calls == [True] and torch.equal(nb, idx)
        S = _scores64(O, qfeat, net.full_feat, "euclidean")
        _check(idx, val, S, 5)
        for mode in ("knn", "hnsw"):
            out = net.predict(xq, mode)
            assert calls[-1] is True
            nb3 = net.get_neighbors(xq, 3)
            ref = torch.cat([O.nw_head_f64(qfeat[b:b + 1], net.full_feat[nb3[b]], net.full_y[nb3[b]], n_classes)
                             for b in range(len(xq))])
            atol = max(3e-5, 3e-6 * S.abs().max().item())
            np.testing.assert_allclose(out.cpu().numpy(), ref.cpu().numpy(), rtol=RTOL, atol=atol)
        n = len(calls)
        assert net.get_neighbors(xq, 33).shape == (len(xq), 33) and net.get_neighbors(xq).shape == (len(xq), N)
        assert len(calls) == n, "k > 32 and k = None take the existing route"
    from nwhead_amd.nwhead.nw import NWNet
    with pytest.raises(ValueError):
        NWNet(net.featurizer, n_classes, full_precision="fp32", search_precision="fp16")


def test_nwnet_shared_support_form(dev, ops, O, monkeypatch):
    """knn_per_query=False: the neighbours of all queries pooled into one support, selected by the rounded search."""
    net, xq, n_classes = _net(full_precision="fp16", search_precision="fp16")
    with torch.no_grad():
        qfeat = net.featurizer(xq)
        nb = net.get_neighbors(xq, 3).reshape(-1)
        out = net.predict(xq, "knn")
    ref = O.nw_head_f64(qfeat, net.full_feat[nb], net.full_y[nb], n_classes)
    np.testing.assert_allclose(out.cpu().numpy(), ref.cpu().numpy(), rtol=RTOL, atol=3e-5)


# ------------------------------------------------------------------------------------------------------------ ShardedBank
def _close(out, ref):
    return bool(((out.double() - ref).abs() <= 2e-5 + 1e-5 * ref.abs()).all())


@pytest.mark.parametrize("k", [1, 10])
@pytest.mark.parametrize("G", [1, 2, 3])
def test_sharded_bank(dev, ops, O, monkeypatch, G, k):
    """Shards emulated in one process as test_sharded_knn_gpu._emulated does: G ShardedBanks of world 1 with explicit
    row_lo, their knn_partial buffers stacked the way the all-gather leaves them, then ops.nw_knn_merge."""
    from nwhead_amd.sharded import ShardedBank, shard_bounds
    C, B, N, d = 9, 33, 1001, 192
    g = torch.Generator().manual_seed(33 * 7919 + 1001 * 31 + 192)
    q, s = torch.randn(B, d, generator=g).to(dev), torch.randn(N, d, generator=g).to(dev)
    sy = torch.randint(0, C, (N,), generator=g).to(dev)
    S = _scores64(O, q, s, "euclidean")
    built = []

    class Counting(ops.SplitBank):
        def __init__(self, *a, **kw):
            built.append(kw.get("precision", "fp32"))
            super().__init__(*a, **kw)

    monkeypatch.setattr(ops, "SplitBank", Counting)
    bounds = [0] + [shard_bounds(N, G, r)[1] for r in range(G)]
    banks = [ShardedBank(s[lo:hi], sy[lo:hi], C, row_lo=lo, precision="fp16", search_precision="fp16")
             for lo, hi in zip(bounds[:-1], bounds[1:])]
    for _ in range(2):
        st = torch.stack([bank.knn_partial(q, k).view(3, B, k) for bank in banks])
        idx, val, lab, out = ops.nw_knn_merge(st[:, 0].view(torch.float32), st[:, 1], st[:, 2], k, C)
    torch.cuda.synchronize()
    assert built == ["fp16"] * G, "one bank per shard, across construction and two searches"
    _check(idx, val, S, k)
    assert torch.equal(lab, sy[idx])
    w = torch.softmax(torch.gather(S, 1, idx), dim=1)
    ref = torch.log(torch.zeros(B, C, dtype=torch.float64, device=dev).scatter_add_(1, sy[idx], w) + 1e-12)
    assert _close(out, ref), float((out.double() - ref).abs().max())
    if G == 1:
        assert torch.equal(banks[0].neighbors(q, k), idx) and torch.equal(banks[0].predict_knn(q, k), out)
    with pytest.raises(ValueError):
        ShardedBank(s, sy, C, precision="fp32", search_precision="fp16")
