"""nw_knn_merge_f32 / ops.nw_knn_merge alone, on synthetic candidates: the cross-shard G-way merge of sorted per-shard
candidate lists to the k best per query (score descending, equal scores by ascending global row) and the per-query k-NN head
over the winners.

The scores are drawn from 7 floats, so ties inside and across shards are the rule; rows are unique global integers (0 and
2^31 - 1 among them); lists are truncated with no-element slots, one shard is wholly empty, and the three arrays sit in
buffers with a stride between shards that is not B * kc.  The selection must equal numpy's lexsort((row, -val))[:k] exactly
(rows, the bits of the values, labels); the log-probabilities must agree with an fp64 evaluation of the formula and with
ops.nw_aggregate on the merged arrays to the project's tolerance (1e-5 relative + 2e-5 absolute)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

VALUES = np.array([-3.5, -1.25, -1.0, 0.0, 0.5, 2.0, 7.75], dtype=np.float32)
CLASSES = (1, 7, 200)
LOG_EPS = float(np.log(np.float32(1e-12)))
# output sentinels: NaN for the floats; -7 for the integers (-1 is what a missing neighbour legitimately gets)
SENTINEL = -7


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from nwhead_amd import ops
    return ops


@pytest.fixture(scope="module")
def lib():
    from nwhead_amd import _lib
    return _lib.load()


def _candidates(G, B, kc, seed, short=False):
    """(vals, rows, labels) as (G, B, kc) numpy arrays obeying the contract.  short: few valid candidates per query (fewer
    than kc in total for most, none at all for the last query)."""
    rng = np.random.default_rng(seed)
    vals = np.full((G, B, kc), -np.inf, dtype=np.float32)
    rows = np.full((G, B, kc), -1, dtype=np.int32)
    labels = np.full((G, B, kc), -1, dtype=np.int32)
    empty = G - 1 if G > 1 else -1                        # one shard is wholly empty
    pool_hi = max(4 * G * kc, 64)
    for b in range(B):
        pool = rng.permutation(pool_hi)[:G * kc].astype(np.int64)
        pool[pool == pool.max()] = 2 ** 31 - 1            # the largest row a 31-bit index can be
        pool[pool == pool.min()] = 0
        pool = pool.reshape(G, kc)
        for g in range(G):
            if g == empty:
                continue
            if short:
                n = 0 if b == B - 1 else int(rng.integers(0, 2)) if G > 1 else int(rng.integers(1, max(kc // 2, 1) + 1))
            else:
                n = kc if rng.random() < 0.5 else int(rng.integers(0, kc + 1))    # some lists truncated
            v = VALUES[rng.integers(0, len(VALUES), n)]
            r = pool[g, :n]
            # labels: mostly inside [0, 7), some inside [0, 200) only, some outside every C, some negative
            y = rng.integers(0, 7, n)
            far = rng.random(n)
            y = np.where(far < 0.2, rng.integers(7, 200, n), y)
            y = np.where(far < 0.06, 250, y)
            y = np.where(far < 0.03, -3, y)
            if b == 0:
                y[:] = 3                                  # a query whose neighbours all share one class
            order = np.lexsort((r, -v))                   # best first, equal scores in ascending row order
            vals[g, b, :n], rows[g, b, :n], labels[g, b, :n] = v[order], r[order], y[order]
    return vals, rows, labels


def _expected(vals, rows, labels, k):
    G, B, kc = vals.shape
    idx = np.full((B, k), -1, dtype=np.int64)
    val = np.full((B, k), -np.inf, dtype=np.float32)
    lab = np.full((B, k), -1, dtype=np.int64)
    for b in range(B):
        v, r, y = vals[:, b].reshape(-1), rows[:, b].reshape(-1), labels[:, b].reshape(-1)
        ok = r >= 0
        v, r, y = v[ok], r[ok], y[ok]
        order = np.lexsort((r, -v))[:k]
        n = len(order)
        idx[b, :n], val[b, :n], lab[b, :n] = r[order], v[order], y[order]
    return idx, val, lab


def _head_f64(idx, val, lab, C):
    B, k = idx.shape
    out = np.zeros((B, C), dtype=np.float64)
    for b in range(B):
        ok = idx[b] >= 0
        if ok.any():
            v = val[b, ok].astype(np.float64)
            w = np.exp(v - v.max())
            w /= w.sum()
            for wj, yj in zip(w, lab[b, ok]):
                if 0 <= yj < C:
                    out[b, yj] += wj
    return np.log(out + 1e-12)


def _close(got, ref):
    return np.abs(got - ref) <= 2e-5 + 1e-5 * np.abs(ref)


def _strided(arr, dev, gap):
    """The (G, B, kc) array inside a (G, B*kc + gap) buffer: a stride between shards that is not B * kc."""
    G, B, kc = arr.shape
    t = torch.from_numpy(arr)
    buf = torch.full((G, B * kc + gap), 77, dtype=t.dtype).to(dev)
    view = buf[:, :B * kc].view(G, B, kc)
    view.copy_(t.to(dev))
    return view


def _call(lib, vals, rows, labels, k, C, want_out=True):
    """The C entry with pre-filled outputs: (status, idx, val, lab, out)."""
    G, B, kc = vals.shape
    d = vals.device
    idx = torch.full((B, k), SENTINEL, dtype=torch.int64, device=d)
    lab = torch.full((B, k), SENTINEL, dtype=torch.int64, device=d)
    val = torch.full((B, k), float("nan"), device=d)
    out = torch.full((B, C), float("nan"), device=d) if want_out else None
    rc = lib.nw_knn_merge_f32(vals.data_ptr(), rows.data_ptr(), labels.data_ptr(), G, B, kc, vals.stride(0) if G > 1 else B * kc, k, C,
                              idx.data_ptr(), val.data_ptr(), lab.data_ptr(), None if out is None else out.data_ptr(),
                              torch.cuda.current_stream(d).cuda_stream)
    torch.cuda.synchronize()
    return rc, idx, val, lab, out


def _check_case(dev, ops, lib, G, B, kc, k, short=False):
    nv, nr, nl = _candidates(G, B, kc, seed=G * 1000 + B * 37 + kc * 3 + k, short=short)
    eidx, eval_, elab = _expected(nv, nr, nl, k)
    if not short and k > 1 and B >= 5:
        assert (eval_[:, 1:] == eval_[:, :-1]).any(), "the data holds ties among the winners"
    vals, rows, labels = (_strided(a, dev, gap) for a, gap in ((nv, 5), (nr, 5), (nl, 5)))
    assert G == 1 or vals.stride(0) == B * kc + 5
    for C in CLASSES:
        rc, idx, val, lab, out = _call(lib, vals, rows, labels, k, C)
        assert rc == 0
        idx_n, val_n, lab_n, out_n = idx.cpu().numpy(), val.cpu().numpy(), lab.cpu().numpy(), out.cpu().numpy()
        # every output element is written
        assert not (idx_n == SENTINEL).any() and not (lab_n == SENTINEL).any()
        assert not np.isnan(val_n).any() and not np.isnan(out_n).any()
        # the selection, exactly
        assert np.array_equal(idx_n, eidx)
        assert np.array_equal(val_n.view(np.uint32), eval_.view(np.uint32)), "the bits of the values"
        assert np.array_equal(lab_n, elab)
        # the head: fp64 formula, and nw_aggregate of the merged arrays
        ref = _head_f64(eidx, eval_, elab, C)
        ok = _close(out_n.astype(np.float64), ref)
        assert ok.all(), (C, float(np.abs(out_n - ref).max()))
        some = torch.from_numpy((eidx >= 0).any(axis=1)).to(dev)       # (a query without any neighbour: no softmax to compare)
        if bool(some.any()):
            agg = ops.nw_aggregate(val[some], lab[some], C).cpu().numpy().astype(np.float64)
            assert _close(out_n[some.cpu().numpy()].astype(np.float64), agg).all()
        # query 0: all neighbours in class 3 -- every other class is log(1e-12)
        if (eidx[0] >= 0).any():
            others = np.delete(out_n[0], 3) if C > 3 else out_n[0]
            assert _close(others.astype(np.float64), np.full(others.shape, LOG_EPS)).all() and len(set(others.tolist())) <= 1
            if C > 3:
                assert abs(float(out_n[0, 3])) <= 2e-5            # log(1 + 1e-12)
        # ops.nw_knn_merge: the same arrays
        res = ops.nw_knn_merge(vals, rows, labels, k, C)
        assert all(torch.equal(a, b) for a, b in zip(res, (idx, val, lab, out)))
    res = ops.nw_knn_merge(vals, rows, labels, k)
    assert len(res) == 3 and torch.equal(res[0], idx) and torch.equal(res[1], val) and torch.equal(res[2], lab)
    return eidx


@pytest.mark.parametrize("k", [1, 4, 10, 32])
@pytest.mark.parametrize("B", [1, 5, 67])
@pytest.mark.parametrize("G", [1, 2, 3, 8, 64])
def test_merge_and_head(dev, ops, lib, G, B, k):
    _check_case(dev, ops, lib, G, B, k, k)


@pytest.mark.parametrize("G,B", [(1, 5), (3, 67), (64, 5)])
def test_lists_longer_than_k(dev, ops, lib, G, B):
    _check_case(dev, ops, lib, G, B, 32, 10)


@pytest.mark.parametrize("G,B,k", [(1, 5, 10), (2, 5, 4), (8, 67, 10), (8, 5, 32), (64, 5, 32)])
def test_short_lists(dev, ops, lib, G, B, k):
    """Fewer than k valid candidates: the tail is (-1, -inf, -1) and the head is computed from the valid ones."""
    eidx = _check_case(dev, ops, lib, G, B, k, k, short=True)
    n_valid = (eidx >= 0).sum(axis=1)
    assert n_valid[-1] == 0, "one query has no candidate at all"
    if k > 1:
        assert (n_valid < k).any() and (n_valid > 0).any()
    for b in range(B):
        assert (eidx[b, n_valid[b]:] == -1).all()


def test_dense_buffers_and_determinism(dev, ops, lib):
    """Contiguous (G, B, kc) tensors (stride_g = B * kc), run twice: bit-identical outputs."""
    nv, nr, nl = _candidates(8, 67, 10, seed=5)
    vals, rows, labels = (torch.from_numpy(a).to(dev) for a in (nv, nr, nl))
    a = ops.nw_knn_merge(vals, rows, labels, 10, 200)
    b = ops.nw_knn_merge(vals, rows, labels, 10, 200)
    eidx, eval_, elab = _expected(nv, nr, nl, 10)
    assert np.array_equal(a[0].cpu().numpy(), eidx)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_refusals_launch_nothing(dev, ops, lib, monkeypatch):
    nv, nr, nl = _candidates(2, 5, 32, seed=9)
    vals, rows, labels = (torch.from_numpy(a).to(dev) for a in (nv, nr, nl))

    def untouched(res):
        rc, idx, val, lab, out = res
        assert bool((idx == SENTINEL).all()) and bool((lab == SENTINEL).all())
        assert bool(torch.isnan(val).all()) and bool(torch.isnan(out).all())
        return rc

    assert untouched(_call(lib, vals, rows, labels, 33, 7)) == -2                                  # k = 33
    assert untouched(_call(lib, vals[:, :, :8].contiguous(), rows[:, :, :8].contiguous(),
                           labels[:, :, :8].contiguous(), 10, 7)) == -2                            # kc < k
    big = [torch.from_numpy(np.repeat(a[:1, :, :4], 65, axis=0).copy()).to(dev) for a in (nv, nr, nl)]
    assert untouched(_call(lib, big[0], big[1], big[2], 4, 7)) == -2                               # G = 65
    st = torch.cuda.current_stream(dev).cuda_stream
    idx = torch.full((5, 4), SENTINEL, dtype=torch.int64, device=dev)
    ptrs = [vals.data_ptr(), rows.data_ptr(), labels.data_ptr()]
    for null in range(3):                                                                          # a null input
        p = [None if i == null else x for i, x in enumerate(ptrs)]
        assert lib.nw_knn_merge_f32(p[0], p[1], p[2], 2, 5, 32, 160, 4, 0, idx.data_ptr(), None, None, None, st) == -1
    assert lib.nw_knn_merge_f32(ptrs[0], ptrs[1], ptrs[2], 2, 5, 32, 160, 4, 0, None, None, None, None, st) == -1   # no idx_out
    assert lib.nw_knn_merge_f32(ptrs[0], ptrs[1], ptrs[2], 2, -5, 32, 160, 4, 0, idx.data_ptr(), None, None, None, st) == -1
    assert lib.nw_knn_merge_f32(ptrs[0], ptrs[1], ptrs[2], 2, 5, 32, 159, 4, 0, idx.data_ptr(), None, None, None, st) == -1
    torch.cuda.synchronize()
    assert bool((idx == SENTINEL).all())

    # the tensor-level entry refuses the same shapes without reaching the library
    from nwhead_amd import _lib
    real, calls = _lib.load(), []

    class Spy:
        def __getattr__(self, name):
            if name == "nw_knn_merge_f32":
                return lambda *a: (calls.append(a[3:9]), real.nw_knn_merge_f32(*a))[1]
            return getattr(real, name)

    monkeypatch.setattr(_lib, "_lib", Spy())
    for bad in ((vals, rows, labels, 33), (vals[:, :, :8].contiguous(), rows[:, :, :8].contiguous(),
                                           labels[:, :, :8].contiguous(), 10), (big[0], big[1], big[2], 4)):
        with pytest.raises(ops.NWHipError):
            ops.nw_knn_merge(*bad)
    assert not calls
    with pytest.raises(ops.NWHipError):
        ops.nw_knn_merge(vals.cpu(), rows.cpu(), labels.cpu(), 4)
    ops.nw_knn_merge(vals, rows, labels, 4)
    assert calls == [(2, 5, 32, 160, 4, 0)]
