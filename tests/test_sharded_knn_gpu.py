"""Neighbour search and per-query k-nearest prediction over a sharded bank with the real kernels.

Shards are emulated in one process: G ShardedBanks of world 1 with explicit row_lo, their knn_partial buffers stacked the
way the all-gather would leave them, then ops.nw_knn_merge -- exactly what ShardedBank.neighbors / predict_knn do after the
collective.  Every case runs with and without NW_SPLIT_ALWAYS=1, so the shards go through the fused search (nw_knn_f32)
once and through the score matrix once.  One test runs two real ranks over gloo on one device.

Checks are against fp64 (the assertions of test_knn_fused_gpu.test_against_fp64_distances: the project's 3e-5 score bound)
and, for the head, against the fp64 reference head evaluated per query on its own returned rows (1e-5 relative + 2e-5
absolute)."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

C = 9


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from nwhead_amd import ops
    return ops


@pytest.fixture(params=[False, True], ids=["default", "split_always"])
def split_always(request, monkeypatch):
    if request.param:
        monkeypatch.setenv("NW_SPLIT_ALWAYS", "1")
    else:
        monkeypatch.delenv("NW_SPLIT_ALWAYS", raising=False)
    return request.param


def _bounds(N, G):
    from nwhead_amd.sharded import shard_bounds
    return [0] + [shard_bounds(N, G, g)[1] for g in range(G)]


def _emulated(ops, q, s, sy, bounds, k, kind="euclidean", n_classes=None):
    """What G ranks would compute: each shard's packed candidates, stacked, merged."""
    from nwhead_amd.sharded import ShardedBank
    B = q.shape[0]
    bufs = []
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        bank = ShardedBank(s[lo:hi], sy[lo:hi], C, kind=kind, row_lo=lo)
        assert bank.row_lo == lo and bank.n_total == hi - lo
        buf = bank.knn_partial(q, k)
        assert buf.dtype == torch.int32 and buf.shape == (3 * B * k,)
        bufs.append(buf.view(3, B, k))
    st = torch.stack(bufs)                                           # (G, 3, B, k): stride between shards 3 B k
    return ops.nw_knn_merge(st[:, 0].view(torch.float32), st[:, 1], st[:, 2], k, n_classes)


def _check_fp64(idx, val, d64, N, k):
    """The assertions of test_against_fp64_distances."""
    B = idx.shape[0]
    assert idx.shape == (B, k) and idx.dtype == torch.int64 and int(idx.min()) >= 0 and int(idx.max()) < N
    assert all(len(set(r)) == k for r in idx.tolist()), "rows are distinct"
    assert bool((val[:, 1:] <= val[:, :-1]).all()), "values are non-increasing"
    kth = torch.sort(d64, dim=1).values[:, k - 1:k]
    got = torch.gather(d64, 1, idx)
    assert float((got - kth).max()) <= 3e-5
    assert float((val.double() + got).abs().max()) <= 3e-5


def _close(out, ref):
    return bool(((out.double() - ref).abs() <= 2e-5 + 1e-5 * ref.abs()).all())


@pytest.fixture(scope="module")
def random_case(dev):
    """B = 33, N = 1001 (odd-sized shards, N % 4 != 0), d = 64; the fp64 distances computed once."""
    g = torch.Generator().manual_seed(33 * 7919 + 1001 * 31 + 64)
    q, s = torch.randn(33, 64, generator=g).to(dev), torch.randn(1001, 64, generator=g).to(dev)
    sy = torch.randint(0, C, (1001,), generator=g).to(dev)
    d64 = torch.cdist(q.double(), s.double())
    assert float(d64.min()) > 1.0, "no query coincides with a support"
    return q, s, sy, d64


# ---- random data: rows and values against fp64, the head against the fp64 head over the returned rows
@pytest.mark.parametrize("k", [1, 10, 32])
@pytest.mark.parametrize("G", [2, 3, 8])
def test_random_data_against_fp64(dev, ops, split_always, random_case, G, k):
    from oracle import nw_oracle as O
    q, s, sy, d64 = random_case
    N = s.shape[0]
    idx, val, lab, out = _emulated(ops, q, s, sy, _bounds(N, G), k, n_classes=C)
    _check_fp64(idx, val, d64, N, k)
    assert torch.equal(lab, sy[idx]), "global labels"
    ref = O.nw_head_f64(q.cpu(), s[idx].cpu(), sy[idx].cpu(), C)
    assert _close(out.cpu(), ref), float((out.cpu().double() - ref).abs().max())


def test_head_cosine(dev, ops, split_always, random_case):
    from oracle import nw_oracle as O
    q, s, sy, _ = random_case
    cos = torch.nn.functional.normalize(q.double(), dim=1) @ torch.nn.functional.normalize(s.double(), dim=1).T
    idx, val, lab, out = _emulated(ops, q, s, sy, _bounds(s.shape[0], 3), 10, kind="cosine", n_classes=C)
    assert all(len(set(r)) == 10 for r in idx.tolist())
    got = torch.gather(cos, 1, idx)
    kth = torch.sort(cos, dim=1, descending=True).values[:, 9:10]
    assert float((kth - got).max()) <= 3e-5 and float((val.double() - got).abs().max()) <= 3e-5
    ref = O.nw_head_f64(q.cpu(), s[idx].cpu(), sy[idx].cpu(), C, kind="cosine")
    assert _close(out.cpu(), ref), float((out.cpu().double() - ref).abs().max())


# ---- exact ties across shards
def test_exact_ties_across_shards(dev, ops, split_always):
    """The small-integer rows of test_knn_fused_gpu.test_ties_keep_the_lowest_rows_in_order: copies of one row have
    bit-equal scores whatever tile they sit in.  The shard bounds (multiples of 4, so that every shard takes the same score
    route) put the copies 1919 / 1920 and the 40 copies of row 300 (300, 311, ..., 729) into different shards."""
    B, N, d = 8, 2048, 64
    g = torch.Generator().manual_seed(1)     # (a seed whose fp64 scores pass the gap assertion below)
    q, s = torch.randn(B, d, generator=g).to(dev), torch.randn(N, d, generator=g).to(dev)
    g = torch.Generator().manual_seed(3)
    s[[100, 1919, 300]] = torch.randint(-3, 4, (3, d), generator=g).float().to(dev)
    s[101] = s[100]
    s[1920] = s[1919]
    copies = list(range(300, 300 + 40 * 11, 11))
    s[copies] = s[300].clone()
    q[0], q[1], q[2] = s[100], s[1919], s[300]
    sy = (torch.arange(N, device=dev) % C)
    sc64 = -torch.cdist(q.double(), s.double())
    order = torch.argsort(sc64, dim=1, descending=True, stable=True)
    # the other scores among the best 33 are further apart than twice the 3e-5 score bound: fp32 cannot reorder them
    top = torch.gather(sc64, 1, order[:, :33])
    gaps = (top[:, :-1] - top[:, 1:])
    assert float(gaps[gaps > 0].min()) > 1e-4
    for bounds in ([0, 512, 1920, 2048], [0, 304, 308, 1920, 2048]):
        assert all(b % 4 == 0 for b in bounds)
        for k in (32, 1):
            idx, val, lab = _emulated(ops, q, s, sy, bounds, k)
            assert torch.equal(idx, order[:, :k]), "the stable descending argsort of the fp64 scores, cut to k"
            assert torch.equal(lab, sy[idx])
            if k == 32:
                assert idx[0, :2].tolist() == [100, 101] and idx[1, :2].tolist() == [1919, 1920]
                assert idx[2].tolist() == copies[:32]


# ---- small shards
@pytest.mark.parametrize("sizes", [[5] * 8, [3, 0, 7, 5, 7, 8, 3, 7], [25, 0, 1, 2, 0, 9, 2, 1]],
                         ids=["even", "empty_shard", "ragged"])
def test_small_shards(dev, ops, split_always, sizes):
    """G = 8 over N = 40, k = 10: no shard has more than 25 rows (the score route), some have fewer than k, one is empty."""
    from oracle import nw_oracle as O
    assert sum(sizes) == 40 and max(sizes) <= 25 and min(sizes) < 10
    g = torch.Generator().manual_seed(40)
    q, s = torch.randn(6, 64, generator=g).to(dev), torch.randn(40, 64, generator=g).to(dev)
    sy = torch.randint(0, C, (40,), generator=g).to(dev)
    bounds = [0]
    for n in sizes:
        bounds.append(bounds[-1] + n)
    d64 = torch.cdist(q.double(), s.double())
    assert float(d64.min()) > 1.0
    idx, val, lab, out = _emulated(ops, q, s, sy, bounds, 10, n_classes=C)
    _check_fp64(idx, val, d64, 40, 10)
    assert torch.equal(lab, sy[idx])
    ref = O.nw_head_f64(q.cpu(), s[idx].cpu(), sy[idx].cpu(), C)
    assert _close(out.cpu(), ref)


# ---- one rank: the public methods and their limits
def test_single_rank_bank_methods(dev, ops, split_always, random_case):
    from nwhead_amd.sharded import ShardedBank
    from oracle import nw_oracle as O
    q, s, sy, d64 = random_case
    for precision in ("fp32", "fp16"):                     # (an fp16 bank is searched through its fp32 shard)
        bank = ShardedBank(s, sy, C, precision=precision)
        assert bank.row_lo == 0 and bank.n_total == 1001
        idx, val, lab = bank.neighbors(q, 10, return_values=True, return_labels=True)
        _check_fp64(idx, val, d64, 1001, 10)
        assert torch.equal(bank.neighbors(q, 10), idx) and torch.equal(lab, sy[idx])
        out = bank.predict_knn(q, 10)
        ref = O.nw_head_f64(q.cpu(), s[idx].cpu(), sy[idx].cpu(), C)
        assert out.shape == (33, C) and _close(out.cpu(), ref)
    for bad, word in ((33, "32"), (0, "1001")):
        with pytest.raises(ops.NWHipError, match=word):
            bank.neighbors(q, bad)
    small = ShardedBank(s[:7], sy[:7], C)
    with pytest.raises(ops.NWHipError, match="N = 7"):
        small.predict_knn(q, 8)


# ---- two ranks over gloo on one device
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), NW_SPLIT_ALWAYS="1")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import sys
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        from nwhead_amd.sharded import ShardedBank, shard_bounds
        from oracle import nw_oracle as O
        dev = torch.device("cuda:0")
        g = torch.Generator().manual_seed(17)
        B, N, d, k = 33, 1001, 64, 10
        s = torch.randn(N, d, generator=g)
        sy = (torch.arange(N) % C).sort().values
        qs = torch.randn(B, d, generator=g)
        d64 = torch.cdist(qs.double(), s.double())
        assert float(d64.min()) > 1.0
        lo, hi = shard_bounds(N, world, rank)
        bank = ShardedBank(s[lo:hi].to(dev), sy[lo:hi].to(dev), C)
        assert bank.row_lo == lo and bank.n_total == N, "row_lo from the all-gather of the shard sizes"
        assert bank.class_lo is not None and bank.CL < C          # class windows are in use: labels must still be global
        idx, val, lab = bank.neighbors(qs.to(dev), k, return_values=True, return_labels=True)
        out = bank.predict_knn(qs.to(dev), k)
        idx, val, lab, out = idx.cpu(), val.cpu(), lab.cpu(), out.cpu()
        _check_fp64(idx, val, d64, N, k)
        assert torch.equal(lab, sy[idx])
        ref = O.nw_head_f64(qs, s[idx], sy[idx], C)
        assert _close(out, ref)
        q.put((rank, idx.numpy(), val.numpy(), lab.numpy(), out.numpy()))
    finally:
        dist.destroy_process_group()


def test_two_ranks_one_device():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=300) for _ in procs], key=lambda r: r[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert [r[0] for r in res] == [0, 1]
    for a, b in zip(res[0][1:], res[1][1:]):
        assert (a.view("u1") == b.view("u1")).all(), "identical on both ranks, bit for bit"
