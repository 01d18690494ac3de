"""The value head over a resident bank: ops.nw_head_values / ops.BankValues -> the forward's lse pass + nw_fwd_values_f32
(fwd_values.hip), and NWNet.set_support_values / predict_values / predict_loo_values.

Reference: fp64 torch on the CPU, softmax(score + a over the admitted rows) @ values with the scores of
oracle.nw_oracle.scores_f64; dead queries (no admitted row with a finite weight) are 0.

Tolerance.  The project's bank-path bound on log-probabilities (tests/test_head_window_gpu.py) is rtol 1e-5 and atol
eps = max(3e-5, 3e-6 * smax), smax = max |score + a| over the finite entries: a relative error of at most eps on every
softmax weight and the same on the normaliser.  So, elementwise,
    |out - ref| <= (2 eps + 1e-6) * (W_ref @ |values|),
the 1e-6 for the split products and the fp32 accumulation.  Every check prints its largest ratio of error to bound; the
largest over this file measured on an MI355X is 0.040 (dotproduct, (37, 1000, 64, 5), kept class window).
Every fused call runs on a workspace filled with 0xFF beforehand."""
import functools
import math

import numpy as np
import pytest
import torch

import ws_poison

pytestmark = pytest.mark.gpu

NEG_INF = float("-inf")
LS0 = float(np.log(1 / 0.07))
KINDS = ("euclidean", "hypersphere_euclidean", "cosine", "dotproduct", "clip")
# (B, N, d, T): a partial query tile, a ragged last support tile and T padded from 5; three query tiles and T padded to 64;
# the smallest bank the kernels take; more than one column slab
SHAPES = [(37, 1000, 64, 5), (130, 4100, 96, 40), (64, 26, 32, 1), (70, 2048, 64, 288)]
PATTERN = (0.0, math.log(2.0), -3.5, NEG_INF, 0.0, 1.25, -0.5)      # the standard weights of test_head_weighted_gpu.py
DEAD_CLASS = 3
C16 = 16
VALUES, SCORES, WINDOW, WEIGHTED, PLAIN = "nw_fwd_values_f32", "nw_scores_f32", "nw_fwd_window_f32", "nw_fwd_weighted_f32", "nw_fwd_f32"
SPIED = (VALUES, SCORES, WINDOW, WEIGHTED, PLAIN, "nw_aggregate_f32")
WORST = {"ratio": 0.0}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "run with -m gpu on the MI355X box"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from nwhead_amd import ops as o
    assert hasattr(o, "nw_head_values") and hasattr(o, "BankValues"), "the value head is missing"
    return o


@pytest.fixture(autouse=True)
def _no_split_always(monkeypatch):
    monkeypatch.delenv("NW_SPLIT_ALWAYS", raising=False)


@pytest.fixture
def launches(monkeypatch):
    """Records the name of every head entry point that is launched: which route a call took."""
    from nwhead_amd import _lib
    lib = _lib.load()
    calls = []

    class Spy:
        def __getattr__(self, name):
            real = getattr(lib, name)
            if name in SPIED:
                return lambda *a: (calls.append(name), real(*a))[1]
            return real

    monkeypatch.setattr(_lib, "_lib", Spy())
    return calls


# ------------------------------------------------------------------------------------------------ data and reference
@functools.lru_cache(maxsize=None)
def _case(B, N, d, T, kind, seed=0):
    """CPU queries, supports, values and the fp64 scores (computed once per case, never written)."""
    from oracle import nw_oracle
    g = torch.Generator().manual_seed(B * 7919 + N * 31 + d + 13 * T + seed)
    q, s, v = torch.randn(B, d, generator=g), torch.randn(N, d, generator=g), torch.randn(N, T, generator=g)
    sc = torch.cat([nw_oracle.scores_f64(q[i:i + 32], s, kind, LS0) for i in range(0, B, 32)])   # (32, N, d) fp64 at a time
    return q, s, v, sc


def _sorted_labels(N, C=C16):
    return (torch.arange(N) % C).sort().values


def _std_logw(sy):
    a = torch.tensor(PATTERN, dtype=torch.float32)[torch.arange(len(sy)) % 7].clone()
    a[sy == DEAD_CLASS] = NEG_INF
    return a


def _class_windows(sy, B, seed=11):
    qy = torch.randint(0, C16, (B,), generator=torch.Generator().manual_seed(seed))
    return torch.searchsorted(sy, qy), torch.searchsorted(sy, qy, right=True)


def _admitted(N, lo, hi, exclude):
    cols = torch.arange(N)
    inside = (cols >= lo.clamp(0, N)[:, None]) & (cols < hi.clamp(0, N)[:, None])
    return ~inside if exclude else inside


def _reference(sc, v, a=None, lo=None, hi=None, exclude=False):
    """(ref, bound, dead, lse) in fp64: W = softmax over the admitted rows of score + a (a dead query: W = 0); .eps of the
    last call: the head's own absolute tolerance at these scores."""
    x = sc.clone() if a is None else sc + a.double()
    if lo is not None:
        x = x.masked_fill(~_admitted(sc.shape[1], lo, hi, exclude), NEG_INF)
    finite = torch.isfinite(x)
    dead = ~finite.any(1)
    smax = x[finite].abs().max().item() if finite.any() else 0.0
    eps = _reference.eps = max(3e-5, 3e-6 * smax)
    W = torch.softmax(x, 1).masked_fill(dead[:, None], 0.0)
    v = v.double()
    return W @ v, (2 * eps + 1e-6) * (W @ v.abs()), dead, torch.logsumexp(x, 1).masked_fill(dead, NEG_INF)


def _within(out, ref, bound, what):
    assert out.shape == ref.shape and out.dtype == torch.float32 and bool(torch.isfinite(out).all()), what
    err = (out.cpu().double() - ref).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf), err)).max().item()
    WORST["ratio"] = max(WORST["ratio"], ratio)
    print(f"{what}: largest error / bound = {ratio:.4g}   (largest so far in this file {WORST['ratio']:.4g})")
    assert bool((err <= bound).all()), (what, ratio)


def _poison(dev, B, N, d, Tp):
    from nwhead_amd import _lib
    need = max(ws_poison.fwd_workspace_bytes(B, N, d, 1), int(_lib.load().nw_fwd_values_workspace_bytes(B, N, d, Tp, 0)))
    assert need > 0 and ws_poison.poison_cached_workspaces(need, dev) >= need


def _run(ops, dev, q, s, bank, vals, kind, poison_shape, **kw):
    _poison(dev, *poison_shape)
    ls = torch.tensor(LS0, device=dev) if kind == "clip" else None
    return ops.nw_head_values(q, s, bank, vals, kind, ls, **kw)


# ------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", KINDS)
def test_parity(dev, ops, launches, kind, shape):
    B, N, d, T = shape
    q, s, v, sc = _case(B, N, d, T, kind)
    sy = _sorted_labels(N)
    qd, sd, vd = q.to(dev), s.to(dev), v.to(dev)
    bank = ops.SplitBank(sd, labels=sy.to(dev))
    vals = ops.BankValues(vd, bank)
    assert vals.T == T and vals.width == T + (-T) % 32 and vals.matches(vd) and not vals.stale()
    lo, hi = _class_windows(sy, B)
    a = _std_logw(sy)
    win = (lo.to(dev), hi.to(dev))
    variants = [("plain", {}, {}),
                ("kept class window", dict(row_window=win), dict(lo=lo, hi=hi)),
                ("excluded window", dict(row_window=win, exclude=True), dict(lo=lo, hi=hi, exclude=True)),
                ("weights", dict(row_logw=a.to(dev)), dict(a=a)),
                ("window and weights", dict(row_window=win, row_logw=a.to(dev)), dict(a=a, lo=lo, hi=hi))]
    for name, kw, rkw in variants:
        n0 = len(launches)
        out, lse = _run(ops, dev, qd, sd, bank, vals, kind, (B, N, d, vals.width), return_lse=True, **kw)
        assert launches[n0:] == [WEIGHTED if "row_logw" in kw else WINDOW, VALUES], (name, launches[n0:])
        ref, bound, dead, ref_lse = _reference(sc, v, **rkw)
        _within(out, ref, bound, f"{kind} {shape} {name}")
        assert bool((out.cpu()[dead] == 0).all()) and bool((lse.cpu()[dead] == NEG_INF).all())
        assert dead.any() == (name == "window and weights")          # the queries of the class that is switched off
        np.testing.assert_allclose(lse.cpu()[~dead].double().numpy(), ref_lse[~dead].numpy(), rtol=1e-5, atol=_reference.eps)
    # a raw tensor is prepared on the fly: the same bits
    assert torch.equal(_run(ops, dev, qd, sd, bank, vd, kind, (B, N, d, vals.width)), _run(ops, dev, qd, sd, bank, vals, kind, (B, N, d, vals.width)))


# ------------------------------------------------------------------------------------------------ 2. chunks, through ctypes
@pytest.mark.parametrize("row_chunks", [1, 3, 7])
def test_forced_chunks_agree_and_repeat_bit_for_bit(dev, ops, row_chunks):
    from nwhead_amd import _lib
    lib = _lib.load()
    B, N, d, T = 37, 1000, 64, 5
    q, s, v, sc = _case(B, N, d, T, "euclidean")
    sy = _sorted_labels(N)
    a = _std_logw(sy)
    lo, hi = _class_windows(sy, B)
    qd, sd = q.to(dev), s.to(dev)
    bank = ops.SplitBank(sd)
    vals = ops.BankValues(v.to(dev), bank)
    ad, lod, hid = a.to(dev), lo.to(dev).int(), hi.to(dev).int()
    _, lse = ops.nw_head_values(qd, sd, bank, vals, row_window=(lod, hid), exclude=True, row_logw=ad, return_lse=True)
    Tp = vals.width
    need = int(lib.nw_fwd_values_workspace_bytes(B, N, d, Tp, row_chunks))
    assert need > 0
    st = torch.cuda.current_stream(dev).cuda_stream
    outs = []
    for _ in range(2):
        ws = ws_poison.poisoned_workspace(need, dev)
        out = torch.full((B, Tp), float("nan"), device=dev)
        rc = lib.nw_fwd_values_f32(qd.data_ptr(), bank.split.data_ptr(), bank.scale.data_ptr(), bank.norm2.data_ptr(),
                                   vals.split.data_ptr(), vals.scale.data_ptr(), ad.data_ptr(), lod.data_ptr(), hid.data_ptr(), 1,
                                   lse.data_ptr(), out.data_ptr(), ws.data_ptr(), need, B, N, d, Tp, 0, None, row_chunks, st)
        assert rc == 0
        torch.cuda.synchronize()
        outs.append(out)
    assert torch.equal(outs[0], outs[1])
    assert bool((outs[0][:, T:] == 0).all())                          # the padding columns are exact zeros
    ref, bound, dead, _ = _reference(sc, v, a=a, lo=lo, hi=hi, exclude=True)
    _within(outs[0][:, :T], ref, bound, f"row_chunks={row_chunks}")


# ------------------------------------------------------------------------------------------------ 3. leave-one-out
def test_leave_one_out_is_applied_before_the_softmax(dev, ops):
    B, N, d, T = 37, 1000, 64, 5
    _, s, v, _ = _case(B, N, d, T, "euclidean")
    from oracle import nw_oracle
    rows = torch.arange(B) * 27                                       # every query a copy of a bank row, at distance 0
    q = s[rows].clone()
    sc = nw_oracle.scores_f64(q, s, "euclidean")
    sd = s.to(dev)
    bank = ops.SplitBank(sd)
    out = _run(ops, dev, q.to(dev), sd, bank, v.to(dev), "euclidean", (B, N, d, 32),
               row_window=(rows.to(dev), rows.to(dev) + 1), exclude=True)
    ref, bound, dead, _ = _reference(sc, v, lo=rows, hi=rows + 1, exclude=True)
    assert not dead.any()
    _within(out, ref, bound, "leave-one-out")
    # the self match dominates the full softmax: were the window applied afterwards, the result would be the row's own value
    full = _run(ops, dev, q.to(dev), sd, bank, v.to(dev), "euclidean", (B, N, d, 32))
    ref_full = _reference(sc, v)[0]       # (not held to the bound: a distance of 0 is where the matmul form of the scores is worst)
    assert (ref_full - v[rows]).abs().max() < 0.3 < (ref - v[rows]).abs().max()
    assert (full.cpu() - v[rows]).abs().max() < 0.3 < (out.cpu() - v[rows]).abs().max()


# ------------------------------------------------------------------------------------------------ 4. normalisation and scaling
def test_constant_values_come_back(dev, ops):
    B, N, d = 70, 2048, 64
    q, s, _, _ = _case(B, N, d, 288, "euclidean")
    sd = s.to(dev)
    bank = ops.SplitBank(sd)
    for c in (1.0, -2.5, 1e3, 3e-4, -7e5):
        out = _run(ops, dev, q.to(dev), sd, bank, torch.full((N, 3), c, device=dev), "euclidean", (B, N, d, 32)).cpu()
        rel = ((out - c) / c).abs().max().item()
        print(f"constant values {c}: largest relative error {rel:.3g}")
        assert rel <= 4e-6


def test_row_magnitudes_over_twelve_decades(dev, ops):
    B, N, d, T = 70, 2048, 64, 40
    q, s, _, sc = _case(B, N, d, 288, "euclidean")
    g = torch.Generator().manual_seed(21)
    mag = 10.0 ** (torch.rand(N, generator=g) * 12 - 6)               # 1e-6 .. 1e6, random per row
    v = torch.randn(N, T, generator=g) * mag[:, None]
    sd = s.to(dev)
    bank = ops.SplitBank(sd)
    out = _run(ops, dev, q.to(dev), sd, bank, v.to(dev), "euclidean", (B, N, d, 64))
    ref, bound, _, _ = _reference(sc, v)
    _within(out, ref, bound, "row magnitudes 1e-6 .. 1e6")
    # rows in ascending magnitude: every tile raises the running exponent and rescales the accumulators
    order = mag.argsort()
    v2 = torch.randn(N, T, generator=g) * mag[order][:, None]
    out = _run(ops, dev, q.to(dev), sd, bank, v2.to(dev), "dotproduct", (B, N, d, 64))
    from oracle import nw_oracle
    ref, bound, _, _ = _reference(nw_oracle.scores_f64(q, s, "dotproduct"), v2)
    _within(out, ref, bound, "row magnitudes ascending")


# ------------------------------------------------------------------------------------------------ 5. agreement with the head
@pytest.fixture(scope="module")
def absent(dev, ops):
    """What the library writes for a class that no row carries (logf(0 + 1e-12f) on the device)."""
    g = torch.Generator().manual_seed(3)
    s, q = torch.randn(64, 32, generator=g).to(dev), torch.randn(4, 32, generator=g).to(dev)
    sy = torch.zeros(64, dtype=torch.int64, device=dev)
    v = ops.nw_head(q, s, sy, 2, support_cache=ops.SplitBank(s, labels=sy))[0, 1].item()
    assert abs(v - math.log(1e-12)) < 4e-6
    return v


def test_one_hot_values_reproduce_the_head(dev, ops, absent):
    B, N, d = 37, 1000, 64
    q, s, _, sc = _case(B, N, d, 5, "euclidean")
    sy = _sorted_labels(N)
    qd, sd, syd = q.to(dev), s.to(dev), sy.to(dev)
    bank = ops.SplitBank(sd, labels=syd)
    vals = ops.BankValues(torch.nn.functional.one_hot(syd, C16).float(), bank)
    a = _std_logw(sy)
    lo, hi = _class_windows(sy, B)
    for name, kw in (("weights", dict(row_window=None, row_logw=a.to(dev))),
                     ("excluded window", dict(row_window=(lo.to(dev), hi.to(dev)), exclude=True)),
                     ("window and weights", dict(row_window=(lo.to(dev), hi.to(dev)), row_logw=a.to(dev)))):
        _poison(dev, B, N, d, 32)
        got = ops.nw_head_values(qd, sd, bank, vals, log=True, **kw)
        head = ops.nw_head_window(qd, sd, syd, C16, bank, **kw)
        x = sc if "row_logw" not in kw else sc + a.double()
        smax = x[torch.isfinite(x)].abs().max().item()
        np.testing.assert_allclose(got.cpu().double().numpy(), head.cpu().double().numpy(), rtol=1e-5, atol=max(3e-5, 3e-6 * smax),
                                   err_msg=name)
        if "row_logw" in kw:      # a class with no admitted row: the library's absent-class value, exactly
            assert bool((got[:, DEAD_CLASS] == absent).all()) and bool((head[:, DEAD_CLASS] == absent).all())
        if name == "window and weights":
            dead = torch.searchsorted(sy, torch.tensor(DEAD_CLASS)) == lo
            assert dead.any() and bool((got.cpu()[dead] == absent).all())
            lin, lse = ops.nw_head_values(qd, sd, bank, vals, return_lse=True, **kw)
            assert bool((lin.cpu()[dead] == 0.0).all()) and bool((lse.cpu()[dead] == NEG_INF).all())


# ------------------------------------------------------------------------------------------------ 6. routes
def test_routes(dev, ops, launches):
    B, N, d, T = 37, 1000, 64, 5
    q, s, v, sc = _case(B, N, d, T, "euclidean")
    sy = _sorted_labels(N)
    a = _std_logw(sy)
    lo, hi = _class_windows(sy, B)
    qd, sd, vd, ad, win = q.to(dev), s.to(dev), v.to(dev), a.to(dev), (lo.to(dev), hi.to(dev))
    ref, bound, _, _ = _reference(sc, v, a=a, lo=lo, hi=hi, exclude=True)
    kw = dict(row_window=win, exclude=True, row_logw=ad)
    # fused: the lse pass and the value kernel, no score matrix
    bank = ops.SplitBank(sd, labels=sy.to(dev))
    _within(ops.nw_head_values(qd, sd, bank, vd, **kw), ref, bound, "fused")
    assert launches == [WEIGHTED, VALUES]
    # matrix: an fp16 bank, a bank from unsorted labels (it keeps a class-sorted copy)
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(2))
    for name, mbank in (("fp16 bank", ops.SplitBank(sd, labels=sy.to(dev), precision="fp16")),
                        ("unsorted labels", ops.SplitBank(sd, labels=sy[perm].to(dev)))):
        del launches[:]
        out, lse = ops.nw_head_values(qd, sd, mbank, vd, return_lse=True, **kw)
        assert SCORES in launches and VALUES not in launches, (name, launches)
        _within(out, ref, bound, f"matrix route, {name}")
        vals = ops.BankValues(vd, mbank)
        assert torch.equal(ops.nw_head_values(qd, sd, mbank, vals, **kw), out)
    # ... and N = 20, below the tile kernels; with dead queries (the kept window of a class that is switched off)
    N2 = 20
    s2, v2, sc2 = s[:N2].contiguous(), v[:N2].contiguous(), sc[:, :N2]
    a2 = torch.tensor(PATTERN)[torch.arange(N2) % 7].clone()
    lo2, hi2 = torch.arange(B) % N2, torch.arange(B) % N2 + 1 + (torch.arange(B) % 3)
    ref2, bound2, dead2, _ = _reference(sc2, v2, a=a2, lo=lo2, hi=hi2)
    assert dead2.any() and not dead2.all()
    del launches[:]
    s2d = s2.to(dev)
    out2, lse2 = ops.nw_head_values(qd, s2d, ops.SplitBank(s2d), v2.to(dev), row_window=(lo2.to(dev), hi2.to(dev)), row_logw=a2.to(dev),
                                    return_lse=True)
    assert (SCORES in launches or PLAIN in launches) and VALUES not in launches      # ops.nw_scores, whichever entry it takes
    _within(out2, ref2, bound2, "matrix route, N = 20")
    assert bool((out2.cpu()[dead2] == 0).all()) and bool((lse2.cpu()[dead2] == NEG_INF).all())
    logged = ops.nw_head_values(qd, s2d, ops.SplitBank(s2d), v2.to(dev), row_window=(lo2.to(dev), hi2.to(dev)), row_logw=a2.to(dev), log=True)
    assert (logged.cpu()[dead2] - math.log(1e-12)).abs().max() < 4e-6


def test_stale_values_and_grad_inputs_are_refused(dev, ops, launches):
    B, N, d, T = 37, 1000, 64, 5
    q, s, v, _ = _case(B, N, d, T, "euclidean")
    qd, sd, vd = q.to(dev), s.to(dev), v.to(dev).clone()
    bank = ops.SplitBank(sd)
    vals = ops.BankValues(vd, bank)
    before = ops.nw_head_values(qd, sd, bank, vals)
    vd[0, 0] += 1.0                                                   # written since: the prepared object is REFUSED, not rebuilt
    assert vals.stale() and not vals.matches(vd)
    n0 = len(launches)
    with pytest.raises(ValueError, match="written since"):
        ops.nw_head_values(qd, sd, bank, vals)
    assert len(launches) == n0
    assert not torch.equal(ops.nw_head_values(qd, sd, bank, ops.BankValues(vd, bank)), before)
    # inference only: nothing is detached silently
    a = torch.zeros(N, device=dev)
    for kw in (dict(q=qd.clone().requires_grad_(True)), dict(values=vd.clone().requires_grad_(True)),
               dict(values=ops.BankValues(vd.clone().requires_grad_(True), bank)), dict(row_logw=a.clone().requires_grad_(True))):
        args = dict(q=qd, values=vd, row_logw=a)
        args.update(kw)
        n0 = len(launches)
        with pytest.raises(ops.NWHipError, match="nw_scores"):
            ops.nw_head_values(args["q"], sd, bank, args["values"], row_logw=args["row_logw"])
        assert len(launches) == n0
        with torch.no_grad():                                         # grad mode off: served
            assert ops.nw_head_values(args["q"], sd, bank, args["values"], row_logw=args["row_logw"]).shape == (B, T)
    with pytest.raises(ValueError, match="value rows"):
        ops.BankValues(vd[:-1], bank)


# ------------------------------------------------------------------------------------------------ 7. NWNet
def _net(dev, **kw):
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


def test_nwnet_values(dev, ops, launches):
    net = _net(dev)
    N, T = net.full_feat.shape[0], 3
    g = torch.Generator().manual_seed(8)
    v = torch.randn(N, T, generator=g).to(dev)
    x = torch.randn(9, 48, generator=g).to(dev)
    with pytest.raises(ops.NWHipError, match="set_support_values"):
        net.predict_values(x)
    with pytest.raises(ValueError, match="one row per bank row"):
        net.set_support_values(v[:-1])
    net.set_support_values(v)
    assert isinstance(net.support_values, ops.BankValues) and net.support_values.T == T
    with torch.no_grad():
        qf = net._eval_featurizer()(x)
    bank = net.full_cache
    out = net.predict_values(x)
    assert launches[-2:] == [WINDOW, VALUES]
    assert torch.equal(out, ops.nw_head_values(qf, net.full_feat, bank, v))
    logged = net.predict_values(x, log=True)      # (log of a negative estimate is NaN, in both)
    assert torch.allclose(logged, ops.nw_head_values(qf, net.full_feat, bank, v, log=True), rtol=0, atol=0, equal_nan=True)
    assert torch.equal(logged[out > 0], torch.log(out[out > 0] + 1e-12))
    # leave_out, and the support weights as a constant
    rows = torch.tensor([3, -1, 399, 0, -1, 17, 200, 201, 40], device=dev)
    lo = rows.clamp(min=0)
    win = (lo, torch.where(rows < 0, lo, lo + 1))
    loo = net.predict_values(x, leave_out=rows)
    assert torch.equal(loo, ops.nw_head_values(qf, net.full_feat, bank, v, row_window=win, exclude=True))
    assert torch.equal(loo[rows < 0], out[rows < 0])
    a = _std_logw(net.full_y.cpu()).to(dev)
    net.set_support_weights(a)
    weighted = net.predict_values(x, leave_out=rows)
    assert torch.equal(weighted, ops.nw_head_values(qf, net.full_feat, bank, v, row_window=win, exclude=True, row_logw=a))
    assert not torch.equal(weighted, loo)
    finite = a.clamp(min=-5.0)
    net.set_support_weights(finite)
    constant = net.predict_values(x, leave_out=rows)
    net.set_support_weights(finite, learnable=True)                   # learnable weights are read detached
    assert torch.equal(net.predict_values(x, leave_out=rows), constant) and not torch.equal(constant, weighted)
    net.set_support_weights(None)
    # the bank's own rows, each without itself
    some = torch.tensor([7, 399, 128, 0], device=dev)
    by_row = ops.nw_head_values(net.full_feat[some], net.full_feat, bank, v, row_window=(some, some + 1), exclude=True)
    assert torch.equal(net.predict_loo_values(some), by_row)
    every = net.predict_loo_values(batch_size=128)
    assert every.shape == (N, T) and torch.equal(every[some], by_row)
    from oracle import nw_oracle
    me = torch.arange(N)
    ref, bound, _, _ = _reference(nw_oracle.scores_f64(net.full_feat.cpu(), net.full_feat.cpu(), "euclidean"), v.cpu(), lo=me, hi=me + 1,
                                  exclude=True)
    _within(every, ref, bound, "predict_loo_values")
    net.return_mask = True
    out_m, mask = net.predict_values(x)
    assert torch.equal(out_m, out) and mask.shape == (9,) and bool(mask.all())
    out_m, mask = net.predict_loo_values(some)
    assert out_m.shape == (4, T) and mask.shape == (4,)
    net.return_mask = False
    # refresh_bank keeps the values (rows keep their identity); a sharded bank is refused; precompute() clears them
    with torch.no_grad():
        net.refresh_bank(some, net.full_feat[some] * 0.5)
    assert net.support_values is not None and net.predict_values(x).shape == (9, T)
    net.sharded_bank = object()
    with pytest.raises(ops.NWHipError, match="sharded"):
        net.predict_values(x)
    with pytest.raises(ops.NWHipError, match="sharded"):
        net.predict_loo_values(some)
    net.sharded_bank = None
    with torch.no_grad():
        net.precompute()
    assert net.support_values is None
    with pytest.raises(ops.NWHipError, match="set_support_values"):
        net.predict_values(x)


def test_nwnet_values_over_an_fp16_bank_take_the_matrix_route(dev, ops, launches):
    net = _net(dev, full_precision="fp16")
    N = net.full_feat.shape[0]
    g = torch.Generator().manual_seed(9)
    v, x = torch.randn(N, 2, generator=g).to(dev), torch.randn(5, 48, generator=g).to(dev)
    net.set_support_values(v)
    del launches[:]
    out = net.predict_values(x)
    assert SCORES in launches and VALUES not in launches
    from oracle import nw_oracle
    with torch.no_grad():
        qf = net._eval_featurizer()(x)
    ref, bound, _, _ = _reference(nw_oracle.scores_f64(qf.cpu(), net.full_feat.cpu(), "euclidean"), v.cpu())
    _within(out, ref, bound, "NWNet, fp16 bank")
