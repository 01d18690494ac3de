"""ops.nw_top_influence / NWNet.explain: the k most helpful and the k most harmful supports of every query with their
influences (util/metric.py:23-50), from two windowed searches over the class-sorted bank and k influence values per list
(nw_knn_window_f32, nw_influence_select_f32) instead of the (B,N) influence matrix of ops.nw_head_influence.

Rows: the masked top-k by score of the bank-route score matrix (helpful: the query's class; harmful: every other class).
Values: ops.nw_head_influence gathered at those rows, and the fp64 oracle for a slice of the queries, with the tolerance
and the comparison condition of test_hip_parity.py::test_forward_plus_influence_in_one_call."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_knn_fused_gpu import _data, dev, ops, split_always  # noqa: F401  (fixtures and the generator, by import)
from test_nwnet_gpu import net_and_g  # noqa: F401  (the tiny model over the support dataset of fixture G5)

pytestmark = pytest.mark.gpu

NEG_INF = float("-inf")
CASES = [(70, 2068, 64, 16), (37, 4100, 96, 200), (256, 2048, 512, 16)]
K = 10


@pytest.fixture(scope="module")
def O():
    from oracle import nw_oracle
    return nw_oracle


_CACHE = {}


def _case(dev, B, N, d, C):
    """Inputs and the matrix route's answer, computed once per shape and left unchanged."""
    key = (B, N, d, C)
    if key not in _CACHE:
        from nwhead_amd import ops
        q, s = _data(dev, B, N, d)
        sy = (torch.arange(N) % C).sort().values.to(dev)
        qy = torch.randint(0, C, (B,), generator=torch.Generator().manual_seed(B + N)).to(dev)
        bank = ops.SplitBank(s, sy)
        out, infl = ops.nw_head_influence(q, s, sy, C, qy, support_cache=bank)
        _, w = ops.nw_head(q, s, sy, C, return_weights=True, support_cache=bank)
        _CACHE[key] = (q, s, sy, qy, bank, out, infl, w)
    return _CACHE[key]


def _masked_topk(ops, q, s, bank, same, k):
    S = ops.nw_scores(q, s, support_cache=bank)
    return (ops.nw_topk(S.masked_fill(~same, NEG_INF), k), ops.nw_topk(S.masked_fill(same, NEG_INF), k))


@pytest.mark.parametrize("B,N,d,C", CASES)
def test_rows(dev, ops, split_always, B, N, d, C):
    q, s, sy, qy, bank, *_ = _case(dev, B, N, d, C)
    r = ops.nw_top_influence(q, s, sy, C, qy, K, support_cache=bank)
    assert r.helpful_rows.shape == r.harmful_rows.shape == r.helpful_infl.shape == r.harmful_infl.shape == (B, K)
    assert r.helpful_rows.dtype == torch.int64 and r.out.shape == (B, C)
    assert bool((sy[r.helpful_rows] == qy[:, None]).all()), "helpful supports have the query's label"
    assert bool((sy[r.harmful_rows] != qy[:, None]).all()), "harmful supports have another label"
    same = sy[None, :] == qy[:, None]
    helpful, harmful = _masked_topk(ops, q, s, bank, same, K)
    assert torch.equal(r.helpful_rows, helpful) and torch.equal(r.harmful_rows, harmful)
    r2, (hl, bl) = ops.nw_top_influence(q, s, sy, C, qy, K, support_cache=bank, return_labels=True)
    assert torch.equal(hl, sy[helpful]) and torch.equal(bl, sy[harmful])
    assert all(torch.equal(a, b) for a, b in zip(r, r2))
    # without a bank of the caller's: one is built for the call
    r3 = ops.nw_top_influence(q, s, sy, C, qy, K)
    assert torch.equal(r3.helpful_rows, helpful) and torch.equal(r3.harmful_rows, harmful)


@pytest.mark.parametrize("B,N,d,C", CASES)
def test_values(dev, ops, O, split_always, B, N, d, C):
    q, s, sy, qy, bank, out, infl, w = _case(dev, B, N, d, C)
    r = ops.nw_top_influence(q, s, sy, C, qy, K, support_cache=bank)
    np.testing.assert_allclose(r.out.cpu().numpy(), out.cpu().numpy(), rtol=1e-5, atol=3e-5)
    rows = torch.cat([r.helpful_rows, r.harmful_rows], dim=1)
    got = torch.cat([r.helpful_infl, r.harmful_infl], dim=1).cpu().numpy()
    same = (sy[rows] == qy[:, None])
    # against the matrix route, where the denominator keeps at least 1e-3 of p
    p = out.exp()[torch.arange(B, device=dev), qy][:, None]
    ref = torch.gather(infl, 1, rows).cpu().numpy()
    ok = ((p - torch.gather(w, 1, rows) * same) > 1e-3 * p).cpu().numpy() & np.isfinite(ref)
    print(f"compared against the matrix route: {ok.mean():.3f} of {ok.size} entries; largest w/p among the helpful ones "
          f"{float((torch.gather(w, 1, r.helpful_rows) / p).max()):.3f}; "
          f"largest difference {np.abs(got[ok] - ref[ok]).max():.3e}")
    np.testing.assert_allclose(got[ok], ref[ok], rtol=2e-4, atol=2e-6)
    assert ok.mean() >= 0.9
    # against the fp64 head with the reference's fp32 influence arithmetic, for a slice of the queries
    n = min(B, 32)
    oref, wref = O.nw_head_f64(q[:n].cpu(), s.cpu(), sy.cpu(), C, return_weights=True)
    iref = O.support_influence_f32(oref.exp().float(), F.one_hot(qy[:n].cpu(), C).float(), wref.float(),
                                   F.one_hot(sy.cpu(), C).float())
    rows_c = rows[:n].cpu()
    p64 = oref.exp().float()[torch.arange(n), qy[:n].cpu()][:, None]
    ref64 = torch.gather(iref, 1, rows_c).numpy()
    ok64 = ((p64 - torch.gather(wref.float(), 1, rows_c) * same[:n].cpu()) > 1e-3 * p64).numpy() & np.isfinite(ref64)
    print(f"compared against fp64: {ok64.mean():.3f} of {ok64.size} entries; "
          f"largest difference {np.abs(got[:n][ok64] - ref64[ok64]).max():.3e}")
    np.testing.assert_allclose(got[:n][ok64], ref64[ok64], rtol=2e-4, atol=2e-6)
    assert ok64.mean() >= 0.9


@pytest.mark.parametrize("B,N,d,C", CASES)
def test_monotone_and_signed(dev, ops, split_always, B, N, d, C):
    q, s, sy, qy, bank, *_ = _case(dev, B, N, d, C)
    r = ops.nw_top_influence(q, s, sy, C, qy, K, support_cache=bank)
    assert bool((r.helpful_infl >= 0).all()) and bool((r.helpful_infl[:, 1:] <= r.helpful_infl[:, :-1]).all())
    assert bool((r.harmful_infl <= 0).all()) and bool((r.harmful_infl[:, 1:] >= r.harmful_infl[:, :-1]).all())


def test_empty_slots(dev, ops, split_always):
    """Class 0 has 3 rows: its queries' helpful lists end in row -1, influence +0.0, label -1."""
    B, N, d, C = 70, 2068, 64, 16
    q, s = _data(dev, B, N, d)
    sy = torch.cat([torch.zeros(3, dtype=torch.int64), 1 + (torch.arange(N - 3) % (C - 1)).sort().values]).to(dev)
    qy = (torch.arange(B) % 4).to(dev)                  # every fourth query is of class 0
    r, (hl, bl) = ops.nw_top_influence(q, s, sy, C, qy, K, return_labels=True)
    small = qy == 0
    assert bool((r.helpful_rows[small][:, :3].sort(dim=1).values == torch.arange(3, device=dev)).all())
    assert bool((r.helpful_rows[small][:, 3:] == -1).all())
    tail = r.helpful_infl[small][:, 3:]
    assert bool((tail == 0).all()) and not bool(torch.signbit(tail).any())
    assert bool((hl[small][:, 3:] == -1).all()) and bool((hl[small][:, :3] == 0).all())
    assert bool((r.helpful_rows[~small] >= 0).all()) and bool((hl[~small] == qy[~small][:, None]).all())
    assert bool((r.harmful_rows >= 0).all()) and bool((bl != qy[:, None]).all()) and bool((bl >= 0).all())
    assert bool((r.helpful_infl >= 0).all()) and bool((r.harmful_infl <= 0).all())


def test_unsorted_labels_and_bad_k(dev, ops):
    B, N, d, C = 8, 400, 64, 10
    q, s = _data(dev, B, N, d)
    qy = torch.zeros(B, dtype=torch.int64, device=dev)
    with pytest.raises(ValueError, match="nw_head_influence"):
        ops.nw_top_influence(q, s, (torch.arange(N) % C).to(dev), C, qy, 5)
    sy = (torch.arange(N) % C).sort().values.to(dev)
    for k in (0, 33):
        with pytest.raises(ops.NWHipError):
            ops.nw_top_influence(q, s, sy, C, qy, k)
    with pytest.raises(ValueError):
        ops.nw_top_influence(q, s, sy, C, qy[:3], 5)


def test_nwnet_explain(net_and_g, ops):
    net, g = net_and_g
    from conftest import T
    x = T(g["xq"]).cuda()
    C = int(g["C"])
    y = (torch.arange(len(x)) % C).cuda()
    with torch.no_grad():
        r = net.explain(x, y)
        qfeat = net._eval_featurizer()(x).detach()
    ref = ops.nw_top_influence(qfeat, net.full_feat, net.full_y, C, y, net.n_neighbors, net.kernel.kind,
                               net.kernel._logit_scale(), support_cache=net.full_cache)
    assert r.helpful_rows.shape == (len(x), net.n_neighbors)
    assert all(torch.equal(a, b) for a, b in zip(r, ref))
    assert bool((net.full_y[r.helpful_rows] == y[:, None]).all()) and bool((net.full_y[r.harmful_rows] != y[:, None]).all())
    with torch.no_grad():
        r5 = net.explain(x, y, k=5)
    assert r5.harmful_rows.shape == (len(x), 5) and torch.equal(r5.harmful_rows[:, :3], r.harmful_rows)
