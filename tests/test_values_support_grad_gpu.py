"""The value head's gradients to the VALUES and the SUPPORT WEIGHTS: ops.nw_head_values_bank(support_grad=True) ->
nw_bwd_values_support_f32 (bwd_values_support.hip), BankValues.refresh and NWNet's learnable ``support_targets``.

Reference: fp64 torch autograd on the CPU over oracle.nw_oracle.scores_f64 (32 queries at a time), softmax(score + a over the
admitted rows) @ values with ``values`` and ``a`` as leaves, the rows masked before the softmax and dead queries set to 0.
Inputs are random normal q, s and values and a random normal upstream gradient (loss = sum(out * gout)).

Bar (the suite's bar for head gradients, test_values_grad_gpu.py): rtol = atol = 1e-4 on values divided by
max(|ref|.max(), 1e-3).  Every comparison prints its normalised error and the module prints the worst one at the end
(DESIGN.md 4.8m).  Every fused call runs on a workspace filled with 0xFF beforehand."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ws_poison

pytestmark = pytest.mark.gpu

NEG_INF = float("-inf")
LS0 = float(np.log(1 / 0.07))
KINDS = ("euclidean", "hypersphere_euclidean", "cosine", "dotproduct", "clip")
# (B, N, d, T), test_values_grad_gpu.py's: a partial query tile, a ragged last support tile, T padded from 5; three query
# tiles, T padded to 64; the smallest bank the regime takes; T' = 288, more than one column slab at either width
SHAPES = [(37, 1000, 64, 5), (130, 4100, 96, 40), (64, 26, 32, 1), (70, 2048, 64, 288)]
SMALL, MID = SHAPES[0], SHAPES[1]
PATTERN = (0.0, math.log(2.0), -3.5, NEG_INF, 0.0, 1.25, -0.5)      # the standard weights of test_head_weighted_gpu.py
DEAD_CLASS = 3
C16 = 16
SUPPORT, BWDV, VALUES, SCORES = "nw_bwd_values_support_f32", "nw_bwd_values_query_f32", "nw_fwd_values_f32", "nw_scores_f32"
SPIED = (SUPPORT, BWDV, VALUES, SCORES, "nw_fwd_window_f32", "nw_fwd_weighted_f32", "nw_fwd_f32", "nw_bwd_query_logw_f32")
WORST = [0.0, ""]
POS_ZERO = 0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "run with -m gpu on the MI355X box"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from nwhead_amd import ops as o
    return o


@pytest.fixture(scope="module", autouse=True)
def report_worst():
    yield
    _CASES.clear()
    print(f"WORST bwd_values_support {WORST[0]:.3e} {WORST[1]}")


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


def close(got, ref, what):
    got, ref = got.detach().cpu().double().numpy(), ref.detach().double().numpy()
    assert got.shape == ref.shape and np.isfinite(got).all(), what
    scale = max(float(np.abs(ref).max()), 1e-3)
    err = float(np.abs(got - ref).max()) / scale
    if err > WORST[0]:
        WORST[:] = [err, what]
    print(f"ERR {err:.3e} {what}")
    np.testing.assert_allclose(got / scale, ref / scale, rtol=1e-4, atol=1e-4, err_msg=what)


def is_pos_zero(t):
    """Every element is +0.0 by its bit pattern."""
    return bool((t.contiguous().view(torch.int32) == POS_ZERO).all())


# ------------------------------------------------------------------------------------------------ data and reference
def _sorted_labels(N, C=C16):
    return (torch.arange(N) % C).sort().values


def _std_logw(sy):
    a = torch.tensor(PATTERN, dtype=torch.float32)[torch.arange(len(sy)) % 7].clone()
    a[sy == DEAD_CLASS] = NEG_INF
    return a


def _admitted(N, lo, hi, exclude):
    cols = torch.arange(N)
    inside = (cols >= lo.clamp(0, N)[:, None]) & (cols < hi.clamp(0, N)[:, None])
    return ~inside if exclude else inside


def weighted_mean_f64(sc, v, a=None, keep=None):
    """fp64 softmax(score + a over the admitted rows) @ v, differentiable in `v` and `a`; a dead query is 0."""
    x = sc if a is None else sc + a
    if keep is not None:
        x = x.masked_fill(~keep, NEG_INF)
    live = torch.isfinite(x).any(dim=1, keepdim=True)
    zero = torch.zeros_like(x)
    return torch.where(live, torch.softmax(torch.where(live, x, zero), dim=1), zero) @ v


def scores_f64(q, s, kind):
    from oracle import nw_oracle
    with torch.no_grad():
        sc = torch.cat([nw_oracle.scores_f64(q[i:i + 32], s, "cosine" if kind == "clip" else kind) for i in range(0, len(q), 32)])
    return sc * math.exp(LS0) if kind == "clip" else sc


def f64_support_grads(sc, v, loss, a=None, keep=None):
    """(d loss / d values, d loss / d a or None) in fp64, `values` and `a` the leaves."""
    vv = v.double().requires_grad_(True)
    aa = None if a is None else a.double().requires_grad_(True)
    out = weighted_mean_f64(sc, vv, aa, keep)
    gr = torch.autograd.grad(loss(out), (vv,) + (() if aa is None else (aa,)))
    return gr[0], (gr[1] if aa is not None else None)


class Case:
    """Inputs of one (shape, kind) on the CPU, the bank on the device, the five variants of the parity test and their fp64
    reference gradients (computed once)."""

    def __init__(self, ops, dev, B, N, d, T, kind):
        g = torch.Generator().manual_seed(B * 7919 + N * 31 + d + 13 * T)
        self.shape, self.kind, self.dev = (B, N, d, T), kind, dev
        self.q, self.s, self.v = torch.randn(B, d, generator=g), torch.randn(N, d, generator=g), torch.randn(N, T, generator=g)
        self.gout = torch.randn(B, T, generator=g)
        self.sy = _sorted_labels(N)
        self.a = _std_logw(self.sy)
        qy = torch.randint(0, C16 - 2, (B,), generator=g)      # (the two last classes: asked for by no query)
        qy[1] = DEAD_CLASS                           # at least one query whose class window holds switched-off rows alone
        self.qy = qy
        self.lo, self.hi = torch.searchsorted(self.sy, qy), torch.searchsorted(self.sy, qy, right=True)
        self.row = (torch.arange(B) * 27 + 5) % N
        self.qd, self.sd, self.vd, self.ad = self.q.to(dev), self.s.to(dev), self.v.to(dev), self.a.to(dev)
        self.bank = ops.SplitBank(self.sd, labels=self.sy.to(dev))
        cls, one = (self.lo.to(dev), self.hi.to(dev)), (self.row.to(dev), self.row.to(dev) + 1)
        self.variants = {
            "plain": ({}, {}),
            "weights": (dict(row_logw=True), dict(a=self.a)),
            "kept class window": (dict(row_window=cls), dict(keep=_admitted(N, self.lo, self.hi, False))),
            "excluded single-row window": (dict(row_window=one, exclude=True), dict(keep=_admitted(N, self.row, self.row + 1, True))),
            "window and weights": (dict(row_window=cls, row_logw=True), dict(a=self.a, keep=_admitted(N, self.lo, self.hi, False))),
        }
        self._sc = self._refs = None

    def ls(self):
        return torch.tensor(LS0, device=self.dev) if self.kind == "clip" else None

    def sc(self):
        if self._sc is None:
            self._sc = scores_f64(self.q, self.s, self.kind)
        return self._sc

    def parity_refs(self):
        if self._refs is None:
            loss = lambda out: (out * self.gout.double()).sum()  # noqa: E731
            self._refs = {name: f64_support_grads(self.sc(), self.v, loss, **rkw) for name, (_, rkw) in self.variants.items()}
        return self._refs


_CASES = {}


def case(ops, dev, shape, kind):
    if (shape, kind) not in _CASES:
        _CASES[(shape, kind)] = Case(ops, dev, *shape, kind)
    return _CASES[(shape, kind)]


def _poison(dev, B, N, d, Tp):
    from nwhead_amd import _lib
    lib = _lib.load()
    need = max(ws_poison.fwd_workspace_bytes(B, N, d, 1), int(lib.nw_fwd_values_workspace_bytes(B, N, d, Tp, 0)),
               int(lib.nw_bwd_values_query_workspace_bytes(B, N, d, Tp, 0)),
               int(lib.nw_bwd_values_support_workspace_bytes(B, N, d, Tp, 0, 1)))
    assert need > 0 and ws_poison.poison_cached_workspaces(need, dev) >= need


def run(ops, c, gout=None, loss=None, values=None, q_grad=False, v_grad=True, log=False, bank=None, **kw):
    """(out, values.grad, row_logw.grad, q.grad) of ops.nw_head_values_bank(support_grad=True) under the upstream gradient
    `gout` (or the scalar loss(out)), on a poisoned workspace.  ``row_logw=True`` stands for the case's standard weights as a
    leaf that requires grad."""
    B, N, d, T = c.shape
    _poison(c.dev, B, N, d, T + (-T) % 32)
    q = c.qd.clone().requires_grad_(q_grad)
    v = (c.vd if values is None else values).clone().requires_grad_(v_grad)
    a = kw.pop("row_logw", None)
    if a is True:
        a = c.ad.clone().requires_grad_(True)
    out = ops.nw_head_values_bank(q, c.sd, c.bank if bank is None else bank, v, c.kind, c.ls(), row_logw=a, log=log,
                                  support_grad=True, **kw)
    _poison(c.dev, B, N, d, T + (-T) % 32)
    if loss is None:
        out.backward(gout.to(c.dev))
    else:
        loss(out).backward()
    return out.detach(), v.grad, None if a is None else a.grad, q.grad


# ------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", KINDS)
def test_parity_with_fp64(ops, dev, launches, kind, shape):
    c = case(ops, dev, shape, kind)
    refs = c.parity_refs()
    for name, (kw, _) in c.variants.items():
        n0 = len(launches)
        out, gv, ga, gq = run(ops, c, c.gout, **kw)
        assert launches[n0:].count(SUPPORT) == 1 and BWDV not in launches[n0:] and SCORES not in launches[n0:], (name, launches[n0:])
        assert gq is None and gv.shape == c.v.shape
        with torch.no_grad():
            kw2 = dict(kw)
            if kw2.pop("row_logw", None):
                kw2["row_logw"] = c.ad
            assert torch.equal(out, ops.nw_head_values(c.qd, c.sd, c.bank, c.vd, c.kind, c.ls(), **kw2)), name
        rv, ra = refs[name]
        close(gv, rv, f"gvalues {kind} {shape} {name}")
        if ra is not None:
            close(ga, ra, f"glogw {kind} {shape} {name}")
        else:
            assert ga is None


# ------------------------------------------------------------------------------------------------ 2. query chunks, repeatability
def _direct(c, dev, chunks, gout, want_gv=True, want_ga=True, guard=64):
    """One ctypes call of nw_bwd_values_support_f32 over the 'window and weights' variant on a NaN workspace, the results
    inside NaN guard zones -> (gvalues (N, Tp), glogw (N,), the guard zones)."""
    from nwhead_amd import _lib, ops
    lib = _lib.load()
    B, N, d, T = c.shape
    Tp = T + (-T) % 32
    vals = ops.BankValues(c.vd, c.bank)
    lod, hid = c.lo.to(dev).int(), c.hi.to(dev).int()
    ls = c.ls()
    with torch.no_grad():
        out, lse = ops.nw_head_values(c.qd, c.sd, c.bank, vals, c.kind, ls, row_window=(lod, hid), row_logw=c.ad, return_lse=True)
    outp = F.pad(out, (0, Tp - T)).contiguous()
    goutp = F.pad(gout.to(dev), (0, Tp - T)).contiguous()
    need = int(lib.nw_bwd_values_support_workspace_bytes(B, N, d, Tp, chunks, int(want_gv)))
    assert need > 0
    ws = ws_poison.poisoned_workspace(need, dev)
    gvbuf = torch.full(((N + 2 * guard) * Tp,), float("nan"), device=dev)
    gabuf = torch.full((N + 2 * guard,), float("nan"), device=dev)
    gv, ga = gvbuf[guard * Tp:(guard + N) * Tp].view(N, Tp), gabuf[guard:guard + N]
    rc = lib.nw_bwd_values_support_f32(c.qd.data_ptr(), c.bank.split.data_ptr(), c.bank.scale.data_ptr(), c.bank.norm2.data_ptr(),
                                       vals.rows.data_ptr(), c.ad.data_ptr(), lod.data_ptr(), hid.data_ptr(), 0, lse.data_ptr(),
                                       outp.data_ptr(), goutp.data_ptr(), gv.data_ptr() if want_gv else None,
                                       ga.data_ptr() if want_ga else None, ws.data_ptr(), need, B, N, d, Tp,
                                       KINDS.index(c.kind), None if ls is None else ls.data_ptr(), chunks,
                                       torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    guards = torch.cat([gvbuf[:guard * Tp], gvbuf[(guard + N) * Tp:], gabuf[:guard], gabuf[guard + N:]])
    return gv, ga, guards


@pytest.mark.parametrize("chunks", [0, 1, 2, 3])
def test_forced_query_chunks_meet_the_bar_and_repeat_bit_for_bit(ops, dev, chunks):
    c = case(ops, dev, MID, "clip")
    B, N, d, T = MID
    assert (B + 63) // 64 == 3                                          # 3: one chunk per query tile, the maximum
    rv, ra = c.parity_refs()["window and weights"]
    res = [_direct(c, dev, chunks, c.gout) for _ in range(2)]
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    close(res[0][0][:, :T], rv, f"gvalues query_chunks={chunks}")
    close(res[0][1], ra, f"glogw query_chunks={chunks}")
    assert is_pos_zero(res[0][0][:, T:])                                # the padding columns of T


# ------------------------------------------------------------------------------------------------ 3. exact zeros
@pytest.mark.parametrize("kind", ["euclidean", "clip"])
def test_rows_nobody_weighs_get_positive_zeros(ops, dev, kind):
    c = case(ops, dev, SMALL, kind)
    B, N, d, T = SMALL
    asked = torch.zeros(C16, dtype=torch.bool)
    asked[c.qy] = True
    unasked = ~asked[c.sy]
    assert unasked.any() and not unasked.all()
    for name in ("kept class window", "window and weights"):
        _, gv, ga, _ = run(ops, c, c.gout, **c.variants[name][0])
        assert is_pos_zero(gv[unasked.to(dev)]), name
        assert float(gv[(~unasked).to(dev)].abs().max()) > 0
        if ga is not None:
            off = unasked | ~torch.isfinite(c.a)
            assert is_pos_zero(ga[off.to(dev)]) and is_pos_zero(gv[(~torch.isfinite(c.a)).to(dev)]), name
    _, gv, ga, _ = run(ops, c, c.gout, row_logw=True)                   # no window: the rows at -inf alone
    off = ~torch.isfinite(c.a)
    assert is_pos_zero(gv[off.to(dev)]) and is_pos_zero(ga[off.to(dev)]) and bool((gv[(~off).to(dev)].abs().amax(1) > 0).all())
    # a batch of dead queries alone (empty kept windows): all-zero gradients
    lo = c.lo.to(dev)
    out, gv, ga, _ = run(ops, c, c.gout, row_window=(lo, lo), row_logw=True)
    assert is_pos_zero(gv) and is_pos_zero(ga) and bool((out == 0).all())


# ------------------------------------------------------------------------------------------------ 4. guards, every element written
@pytest.mark.parametrize("mode", ["both", "values", "weights"])
def test_guards_stay_nan_and_every_element_is_written(ops, dev, mode):
    """The results lie inside NaN zones of 64 rows before and after them and the workspace is NaN (0xFF) first: the zones stay
    NaN, the results are finite.  (gvalues is a dense (N, T') array: its guard columns are the padding columns of T', which
    are written, as exact zeros.)"""
    c = case(ops, dev, SHAPES[3], "euclidean")
    T = c.shape[3]
    for chunks in (0, 2):
        gv, ga, guards = _direct(c, dev, chunks, c.gout, want_gv=mode != "weights", want_ga=mode != "values")
        assert bool(torch.isnan(guards).all())
        if mode != "weights":
            assert bool(torch.isfinite(gv).all()) and is_pos_zero(gv[:, T:])
        else:
            assert bool(torch.isnan(gv).all())
        if mode != "values":
            assert bool(torch.isfinite(ga).all())
        else:
            assert bool(torch.isnan(ga).all())
    rv, ra = c.parity_refs()["window and weights"]
    if mode != "weights":
        close(gv[:, :T], rv, f"gvalues direct, {mode}")
    if mode != "values":
        close(ga, ra, f"glogw direct, {mode}")


# ------------------------------------------------------------------------------------------------ 5. reference-free identities
@pytest.mark.parametrize("kind", KINDS)
def test_column_sums_and_the_weights_sum(ops, dev, kind):
    c = case(ops, dev, MID, kind)
    kw, rkw = c.variants["window and weights"]
    _, gv, ga, _ = run(ops, c, c.gout, **kw)
    live = (rkw["keep"] & torch.isfinite(c.a)[None, :]).any(1)
    assert live.any() and not live.all()
    close(gv.sum(0), c.gout[live].double().sum(0), f"gvalues.sum(0) = sum of gout over live queries, {kind}")
    scale = max(float(c.parity_refs()["window and weights"][1].abs().max()), 1e-3)
    err = abs(float(ga.double().sum())) / scale
    print(f"ERR {err:.3e} glogw.sum() ~ 0, {kind}")
    assert err < 1e-4


# ------------------------------------------------------------------------------------------------ 6. exact scaling
@pytest.mark.parametrize("kind", ["euclidean", "clip"])
def test_scaling_gout_by_a_power_of_two_scales_gvalues_exactly(ops, dev, kind):
    c = case(ops, dev, MID, kind)
    kw = c.variants["weights"][0]
    _, gv, _, _ = run(ops, c, c.gout, **kw)
    assert float(gv.abs().max()) > 0
    for k in (20, -20):
        _, g2, _, _ = run(ops, c, c.gout * 2.0 ** k, **kw)
        want = gv * 2.0 ** k                                            # (ldexp: a product with an exact power of two)
        print(f"k = {k}: {int((g2 != want).sum())} of {g2.numel()} elements differ")
        assert torch.equal(g2, want), f"k = {k}"


# ------------------------------------------------------------------------------------------------ 7. agreement with the class head
def test_one_hot_values_agree_with_the_class_head(ops, dev):
    c = case(ops, dev, SMALL, "euclidean")
    B, N, d, _ = SMALL
    onehot = F.one_hot(c.sy, C16).float()
    target = torch.randint(0, C16, (B,), generator=torch.Generator().manual_seed(4))
    kw = c.variants["excluded single-row window"][0]
    keep = c.variants["excluded single-row window"][1]["keep"]
    a0 = _std_logw(c.sy).clamp(min=-5.0)
    _, ra = f64_support_grads(c.sc(), onehot, lambda out: F.nll_loss(torch.log(out + 1e-12), target, reduction="sum") / B,
                              a=a0, keep=keep)
    a1 = a0.to(dev).requires_grad_(True)
    out = ops.nw_head_values_bank(c.qd, c.sd, c.bank, onehot.to(dev), row_logw=a1, log=True, support_grad=True, **kw)
    F.nll_loss(out, target.to(dev)).backward()
    close(a1.grad, ra, "row_logw.grad, one-hot values, log, nll_loss")
    a2 = a0.to(dev).requires_grad_(True)
    F.nll_loss(ops.nw_head_bank(c.qd, c.sd, c.sy.to(dev), C16, c.bank, row_logw=a2, **kw), target.to(dev)).backward()
    close(a2.grad, ra, "row_logw.grad of nw_head_bank at the same inputs")


# ------------------------------------------------------------------------------------------------ 8. the query gradient's bits
@pytest.mark.parametrize("kind", ["euclidean", "clip"])
def test_query_gradient_is_bit_equal_to_the_call_without_support_grad(ops, dev, launches, kind):
    c = case(ops, dev, MID, kind)
    B, N, d, T = MID
    kw = dict(row_window=(c.lo.to(dev), c.hi.to(dev)))
    ls = None if kind != "clip" else torch.tensor(LS0, device=dev, requires_grad=True)
    q0 = c.qd.clone().requires_grad_(True)
    ops.nw_head_values_bank(q0, c.sd, c.bank, c.vd, kind, ls, row_logw=c.ad, **kw).backward(c.gout.to(dev))
    gls0 = None if ls is None else ls.grad.clone()
    if ls is not None:
        ls.grad = None
    q1, v1, a1 = c.qd.clone().requires_grad_(True), c.vd.clone().requires_grad_(True), c.ad.clone().requires_grad_(True)
    del launches[:]
    ops.nw_head_values_bank(q1, c.sd, c.bank, v1, kind, ls, row_logw=a1, support_grad=True, **kw).backward(c.gout.to(dev))
    assert launches.count(BWDV) == 1 and launches.count(SUPPORT) == 1
    assert torch.equal(q0.grad, q1.grad) and (ls is None or torch.equal(gls0, ls.grad))
    rv, ra = c.parity_refs()["window and weights"]
    close(v1.grad, rv, f"gvalues beside gq, {kind}")
    close(a1.grad, ra, f"glogw beside gq, {kind}")
    # with nothing on the support side requiring grad, the keyword changes nothing
    q2 = c.qd.clone().requires_grad_(True)
    del launches[:]
    ops.nw_head_values_bank(q2, c.sd, c.bank, c.vd, kind, ls, row_logw=c.ad, support_grad=True, **kw).backward(c.gout.to(dev))
    assert SUPPORT not in launches and torch.equal(q2.grad, q0.grad)
    # a BankValues whose source is alive: the gradient goes to the source, in its dtype
    v16 = c.vd.half().requires_grad_(True)
    bv = ops.BankValues(v16, c.bank)
    ops.nw_head_values_bank(c.qd, c.sd, c.bank, bv, kind, c.ls(), support_grad=True).backward(c.gout.to(dev))
    assert v16.grad is not None and v16.grad.dtype == torch.float16 and v16.grad.shape == v16.shape
    del v16
    with pytest.raises(ops.NWHipError, match="is gone"):
        ops.nw_head_values_bank(c.qd, c.sd, c.bank, bv, kind, c.ls(), support_grad=True)
    # the default still refuses, with its own words
    with pytest.raises(ops.NWHipError, match="does not detach silently"):
        ops.nw_head_values_bank(c.qd, c.sd, c.bank, v1, kind, c.ls())


# ------------------------------------------------------------------------------------------------ 9. the weights-only mode
def test_weights_only_mode_is_one_call_and_allocates_nothing_of_size_NxT(ops, dev, launches):
    c = case(ops, dev, MID, "euclidean")
    B, N, d, T = MID
    vals = ops.BankValues(c.vd, c.bank)
    kw = dict(row_window=(c.lo.to(dev), c.hi.to(dev)))
    gout = c.gout.to(dev)
    a = c.ad.clone().requires_grad_(True)
    ops.nw_head_values_bank(c.qd, c.sd, c.bank, vals, row_logw=a, support_grad=True, **kw).backward(gout)   # (workspaces cached)
    a.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    del launches[:]
    ops.nw_head_values_bank(c.qd, c.sd, c.bank, vals, row_logw=a, support_grad=True, **kw).backward(gout)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(dev) - base
    assert launches.count(SUPPORT) == 1 and BWDV not in launches and SCORES not in launches, launches
    print(f"peak allocation of a weights-only step at {MID}: {peak} bytes against N T 4 = {N * T * 4}")
    assert peak < N * T * 4
    close(a.grad, c.parity_refs()["window and weights"][1], "glogw, weights-only mode")


# ------------------------------------------------------------------------------------------------ 10. the matrix routes
def test_matrix_routes(ops, dev, launches):
    c = case(ops, dev, SMALL, "euclidean")
    B, N, d, T = SMALL
    kw = c.variants["window and weights"][0]
    rv, ra = c.parity_refs()["window and weights"]
    fp16 = ops.SplitBank(c.sd, labels=c.sy.to(dev), precision="fp16")
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(3))
    unsorted = ops.SplitBank(c.sd, labels=c.sy[perm].to(dev))          # (only the bank's route depends on the labels)
    assert unsorted.sorted_rows is not None
    for name, bank in (("fp16 bank", fp16), ("unsorted labels", unsorted)):
        del launches[:]
        _, gv, ga, gq = run(ops, c, c.gout, bank=bank, q_grad=True, **kw)
        assert SCORES in launches and SUPPORT not in launches and BWDV not in launches, (name, launches)
        close(gv, rv, f"gvalues matrix route, {name}")
        close(ga, ra, f"glogw matrix route, {name}")
        assert gq is not None and bool(torch.isfinite(gq).all())
    # N = 20, below the tile kernels
    N2 = 20
    s2, v2 = c.s[:N2].contiguous(), c.v[:N2].contiguous()
    a2 = torch.tensor(PATTERN)[torch.arange(N2) % 7].clone()
    lo2, hi2 = torch.arange(B) % N2, torch.arange(B) % N2 + 1 + (torch.arange(B) % 3)
    keep2 = _admitted(N2, lo2, hi2, False)
    rv2, ra2 = f64_support_grads(scores_f64(c.q, s2, "euclidean"), v2, lambda out: (out * c.gout.double()).sum(), a=a2, keep=keep2)
    s2d = s2.to(dev)
    v2d, a2d = v2.to(dev).requires_grad_(True), a2.to(dev).requires_grad_(True)
    del launches[:]
    out = ops.nw_head_values_bank(c.qd, s2d, ops.SplitBank(s2d), v2d, row_window=(lo2.to(dev), hi2.to(dev)), row_logw=a2d,
                                  support_grad=True)
    out.backward(c.gout.to(dev))
    assert SUPPORT not in launches and VALUES not in launches, launches
    close(v2d.grad, rv2, "gvalues matrix route, N = 20")
    close(a2d.grad, ra2, "glogw matrix route, N = 20")


# ------------------------------------------------------------------------------------------------ 11. BankValues.refresh
def test_refresh_gives_the_bits_of_a_new_bankvalues_and_allocates_nothing(ops, dev):
    c = case(ops, dev, SMALL, "euclidean")
    src = c.vd.clone()
    bv = ops.BankValues(src, c.bank)
    ptrs = (bv.rows.data_ptr(), bv.split.data_ptr(), bv.scale.data_ptr())
    with torch.no_grad():
        src.mul_(1.5).add_(0.25)
    assert bv.stale()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    assert bv.refresh() is bv
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated(dev) == base
    assert not bv.stale() and bv.matches(src) and ptrs == (bv.rows.data_ptr(), bv.split.data_ptr(), bv.scale.data_ptr())
    new = ops.BankValues(src, c.bank)
    assert torch.equal(bv.rows, new.rows) and torch.equal(bv.scale, new.scale)
    assert torch.equal(bv.split.view(torch.int32), new.split.view(torch.int32))
    with torch.no_grad():
        assert torch.equal(ops.nw_head_values(c.qd, c.sd, c.bank, bv), ops.nw_head_values(c.qd, c.sd, c.bank, new))
    del src
    with pytest.raises(ops.NWHipError, match="is gone"):
        bv.refresh()


# ------------------------------------------------------------------------------------------------ 12. NWNet
def test_nwnet_learns_soft_labels_and_weights(ops, dev, launches):
    from nwhead_amd.nwhead.nw import NWNet

    class DS(torch.utils.data.Dataset):
        def __init__(self):
            g = torch.Generator().manual_seed(5)
            self.targets = (torch.arange(400) // 40).tolist()
            centres = 4.0 * torch.randn(10, 48, generator=g)
            self.x = centres[torch.tensor(self.targets)] + torch.randn(400, 48, generator=g)

        def __len__(self):
            return 400

        def __getitem__(self, i):
            return self.x[i], self.targets[i]

    torch.manual_seed(0)
    ds = DS()
    net = NWNet(torch.nn.Linear(48, 64), 10, support_dataset=ds, n_shot_full=40, device=dev).to(dev)
    net.eval()
    with torch.no_grad():
        net.precompute()
    net.train()
    N = net.full_feat.shape[0]
    assert "support_targets" not in net.state_dict()
    # one-hot targets, a fifth of them flipped to the next class
    y = net.full_y.clone()
    flipped = torch.arange(N, device=dev) % 5 == 0
    noisy = torch.where(flipped, (y + 1) % 10, y)
    net.set_support_values(F.one_hot(noisy, 10).float() * 0.9 + 0.01, learnable=True)
    assert "support_targets" in net.state_dict() and net.support_targets.shape == (N, 10)
    assert any(p is net.support_targets for p in net.parameters())
    rows = torch.arange(N, device=dev)
    x = ds.x.to(dev)                                               # the dataset's own samples, their clean labels the targets
    clean = F.one_hot(torch.tensor(ds.targets, device=dev), 10).float()
    opt = torch.optim.SGD([net.support_targets], lr=20.0)
    losses = []
    for _ in range(4):
        opt.zero_grad()
        del launches[:]
        out = net.forward_values(x, leave_out=rows, log=True)
        loss = F.kl_div(out, clean, reduction="batchmean")
        loss.backward()
        assert launches.count(SUPPORT) == 1 and SCORES not in launches
        assert net.support_targets.grad is not None and bool(torch.isfinite(net.support_targets.grad).all())
        opt.step()
        with torch.no_grad():
            net.support_targets.clamp_(min=1e-3)
        losses.append(float(loss))
    print("KL over the SGD steps:", losses)
    assert losses[-1] < losses[0]
    # predict_values reads the stepped values (re-prepared in place), detached
    net.eval()
    with torch.no_grad():
        got = net.predict_values(x[:16])
        want = ops.nw_head_values(net._eval_featurizer()(x[:16]), net.full_feat, net.full_cache,
                                  ops.BankValues(net.support_targets.detach().clone(), net.full_cache), net.kernel.kind)
    assert torch.equal(got, want)
    net.train()
    # weights_grad: the default reads learnable weights detached, True passes them with their graph
    net.set_support_weights(torch.zeros(N, device=dev), learnable=True)
    net.zero_grad()
    F.kl_div(net.forward_values(x, leave_out=rows, log=True), clean, reduction="batchmean").backward()
    assert net.support_logw.grad is None and net.support_targets.grad is not None
    net.zero_grad()
    F.kl_div(net.forward_values(x, leave_out=rows, log=True, weights_grad=True), clean, reduction="batchmean").backward()
    assert net.support_logw.grad is not None and float(net.support_logw.grad.abs().max()) > 0
    # precompute() clears the parameter with the values
    net.eval()
    with torch.no_grad():
        net.precompute()
    assert "support_targets" not in net.state_dict() and net.support_values is None
