"""The value head's gradient to the BANK ROWS over a resident bank (bwd_values_bank.hip: nw_bwd_values_bank_support_f32,
ops.nw_head_values_bank(support_grad=True) with `s` requiring grad, NWNet.forward_values after set_bank_learnable()).

Reference: fp64 torch autograd on the CPU of softmax(score + a over the admitted rows) @ values with `s` a leaf, rows masked
before the softmax and dead queries 0.  The scores are the oracle's (oracle.nw_oracle.scores_f64); at a distance of exactly 0
no gradient passes, the convention of head_f64 in test_bank_support_grad_gpu.py.  Inputs are random normal q, s and values
and a random normal upstream gradient (loss = sum(out * gout)).

Bar (the suite's bar for head gradients, test_bwd_query_gpu.py): rtol = atol = 1e-4 on values divided by
max(|ref|.max(), 1e-3).  Every comparison prints its normalised error, and the module prints the worst one at the end
(DESIGN.md 4.8n)."""
import math

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import ws_poison

pytestmark = pytest.mark.gpu

INF = float("inf")
LS0 = float(np.log(1 / 0.07))
KINDS = ("euclidean", "hypersphere_euclidean", "cosine", "dotproduct", "clip")
# (B, N, d, T): a partial query tile, a ragged last support tile, T padded from 5; a padded bank 160 -> 192, three query tiles,
# T padded to 64; the smallest bank of the regime; more than one column slab (544 > 256); nine 32-column steps of the second
# product (T = 288), which exercise its rotation
SHAPES = [(37, 1000, 64, 5), (129, 257, 160, 33), (64, 26, 32, 1), (70, 1000, 544, 40), (33, 4099, 64, 288)]
SMALL, PADDED = SHAPES[0], SHAPES[1]
PATTERN = (0.0, math.log(2.0), -3.5, -INF, 0.0, 1.25, -0.5)         # the standard weights of test_head_weighted_gpu.py
DEAD_CLASS = 3
C16 = 16
ROWS, QUERY, SUPPORT, SCORES = ("nw_bwd_values_bank_support_f32", "nw_bwd_values_query_f32", "nw_bwd_values_support_f32",
                                "nw_scores_f32")
SPIED = (ROWS, QUERY, SUPPORT, SCORES, "nw_fwd_values_f32", "nw_fwd_f32")
WORST = [0.0, ""]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "run with -m gpu on the MI355X box"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from nwhead_amd import ops as o
    return o


@pytest.fixture(scope="module")
def O():
    from oracle import nw_oracle
    return nw_oracle


@pytest.fixture(scope="module", autouse=True)
def report_worst():
    yield
    _CASES.clear()
    print(f"WORST values_bank_support {WORST[0]:.3e} {WORST[1]}")


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
    got, ref = got.detach().cpu().double().numpy(), ref.detach().cpu().double().numpy()
    assert got.shape == ref.shape and np.isfinite(got).all() and np.isfinite(ref).all(), what
    scale = max(float(np.abs(ref).max()), 1e-3)
    err = float(np.abs(got - ref).max()) / scale
    if err > WORST[0]:
        WORST[:] = [err, what]
    print(f"ERR {err:.3e} {what}")
    np.testing.assert_allclose(got / scale, ref / scale, rtol=1e-4, atol=1e-4, err_msg=what)


def is_pos_zero(t):
    """Every element is +0.0 by its bit pattern."""
    return bool((t.contiguous().view(torch.int32) == 0).all())


# ------------------------------------------------------------------------------------------------ data and reference
def scores_f64(O, q, s, kind):
    """The oracle's fp64 scores as a function of the leaf `s` (head_f64 of test_bank_support_grad_gpu.py)."""
    if kind == "clip":
        qn = q / q.norm(dim=-1, keepdim=True).clamp_min(1e-12)
        sn = s / s.norm(dim=-1, keepdim=True).clamp_min(1e-12)
        return math.exp(LS0) * (qn @ sn.t())
    if kind in ("euclidean", "hypersphere_euclidean"):
        # scores_f64's values; its sqrt has the gradient 0 / 0 at a distance of exactly 0, where torch.cdist, backward.hip and
        # the kernels pass no gradient: that convention here
        xq, sx = q[:, None, :], s[None]
        if kind == "hypersphere_euclidean":
            xq = xq / xq.norm(dim=-1, keepdim=True).clamp_min(1e-12)
            sx = sx / sx.norm(dim=-1, keepdim=True).clamp_min(1e-12)
        d2 = (xq - sx).pow(2).sum(-1)
        sc = -torch.where(d2 > 0, torch.where(d2 > 0, d2, torch.ones_like(d2)).sqrt(), torch.zeros_like(d2))
        assert torch.equal(sc.detach(), O.scores_f64(q.detach(), s.detach(), kind, LS0))
        return sc
    return O.scores_f64(q, s, kind, LS0)


def weighted_mean_f64(sc, v, a=None, keep=None):
    """fp64 softmax(score + a over the admitted rows) @ v; a = -inf removes a row, a dead query is 0."""
    if a is not None:
        a = a.double()
        on = (a > -INF)[None, :].expand_as(sc)
        keep = on if keep is None else keep & on
        sc = sc + torch.where(a > -INF, a, torch.zeros_like(a))
    if keep is not None:
        sc = sc.masked_fill(~keep, -INF)
        live = keep.any(dim=1, keepdim=True)
        w = torch.where(live, torch.softmax(torch.where(live, sc, torch.zeros_like(sc)), dim=-1), torch.zeros_like(sc))
    else:
        w = torch.softmax(sc, dim=-1)
    return w @ v.double()


def ref_gs(O, q, s, v, kind, variants, loss):
    """{name: fp64 d loss(out) / d s} for variants {name: dict(a=..., keep=...)}: the score graph is built once."""
    sl = s.double().requires_grad_(True)
    sc = scores_f64(O, q.double(), sl, kind)
    names = list(variants)
    return {name: torch.autograd.grad(loss(weighted_mean_f64(sc, v, **variants[name])), sl, retain_graph=name != names[-1])[0]
            for name in names}


def _sorted_labels(N, C=C16):
    return (torch.arange(N) % C).sort().values


def _std_logw(sy):
    a = torch.tensor(PATTERN, dtype=torch.float32)[torch.arange(len(sy)) % 7].clone()
    a[sy == DEAD_CLASS] = -INF
    return a


def _admitted(N, lo, hi, exclude):
    cols = torch.arange(N)
    inside = (cols >= lo.clamp(0, N)[:, None]) & (cols < hi.clamp(0, N)[:, None])
    return ~inside if exclude else inside


class Case:
    """Inputs of one (shape, kind) on the CPU, the bank on the device, the five variants of the parity test and their fp64
    reference gradients (computed once, the score graph dropped behind them)."""

    def __init__(self, O, ops, dev, B, N, d, T, kind):
        g = torch.Generator().manual_seed(B * 7919 + N * 31 + d + 13 * T)
        self.O, self.shape, self.kind, self.dev = O, (B, N, d, T), kind, dev
        self.q, self.s, self.v = torch.randn(B, d, generator=g), torch.randn(N, d, generator=g), torch.randn(N, T, generator=g)
        if kind == "dotproduct":       # keep |score| O(1..10): the softmax of raw dot products is a one-hot otherwise
            self.q, self.s = self.q * d ** -0.25, self.s * d ** -0.25
        self.gout = torch.randn(B, T, generator=g)
        self.sy = _sorted_labels(N)
        self.a = _std_logw(self.sy)
        qy = torch.randint(0, C16 - 2, (B,), generator=g)      # (the two last classes: asked for by no query)
        qy[1] = DEAD_CLASS                           # a query whose class window holds switched-off rows alone
        self.qy = qy
        self.lo, self.hi = torch.searchsorted(self.sy, qy), torch.searchsorted(self.sy, qy, right=True)
        self.row = (torch.arange(B) * 27 + 5) % N
        self.qd, self.sd, self.vd, self.ad = self.q.to(dev), self.s.to(dev), self.v.to(dev), self.a.to(dev)
        self.bank = ops.SplitBank(self.sd)
        self.vals = ops.BankValues(self.vd, self.bank)
        cls, one = (self.lo.to(dev), self.hi.to(dev)), (self.row.to(dev), self.row.to(dev) + 1)
        self.variants = {
            "plain": ({}, {}),
            "weights": (dict(row_logw=self.ad), dict(a=self.a)),
            "kept class window": (dict(row_window=cls), dict(keep=_admitted(N, self.lo, self.hi, False))),
            "excluded single-row window": (dict(row_window=one, exclude=True), dict(keep=_admitted(N, self.row, self.row + 1, True))),
            "window and weights": (dict(row_window=cls, row_logw=self.ad), dict(a=self.a, keep=_admitted(N, self.lo, self.hi, False))),
        }
        self._refs = None

    def ls(self, grad=False):
        return torch.tensor(LS0, device=self.dev, requires_grad=grad) if self.kind == "clip" else None

    def parity_refs(self):
        if self._refs is None:
            self._refs = ref_gs(self.O, self.q, self.s, self.v, self.kind, {n: r for n, (_, r) in self.variants.items()},
                                lambda out: (out * self.gout.double()).sum())
        return self._refs


_CASES = {}


def case(O, ops, dev, shape, kind):
    if (shape, kind) not in _CASES:
        _CASES[(shape, kind)] = Case(O, ops, dev, *shape, kind)
    return _CASES[(shape, kind)]


def run(ops, c, gout=None, loss=None, q=None, values=None, q_grad=False, s_grad=True, log=False, bank=None, sd=None, ls=None, **kw):
    """(out, s.grad, q.grad) of ops.nw_head_values_bank(support_grad=True) under the upstream gradient `gout` (or the scalar
    loss(out)); the bank's own tensor is the leaf (the bank matches it by address, shape and version)."""
    qd = (c.qd if q is None else q.to(c.dev)).clone().requires_grad_(q_grad)
    s = (c.sd if sd is None else sd).requires_grad_(s_grad)
    s.grad = None
    try:
        out = ops.nw_head_values_bank(qd, s, c.bank if bank is None else bank, c.vals if values is None else values, c.kind,
                                      c.ls() if ls is None else ls, log=log, support_grad=True, **kw)
        if loss is None:
            out.backward(gout.to(c.dev))
        else:
            loss(out).backward()
        return out.detach(), s.grad, qd.grad
    finally:
        s.requires_grad_(False)
        s.grad = None


# ------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", KINDS)
def test_parity_with_fp64(O, ops, dev, launches, kind, shape):
    c = case(O, ops, dev, shape, kind)
    B, N, d, T = shape
    refs = c.parity_refs()
    for name, (kw, _) in c.variants.items():
        n0 = len(launches)
        out, gs, gq = run(ops, c, c.gout, **kw)
        # only the rows learning: the new entry, once, and no other backward call
        seen = launches[n0:]
        assert seen.count(ROWS) == 1 and QUERY not in seen and SUPPORT not in seen and SCORES not in seen, (name, seen)
        assert gq is None and gs.shape == (N, d) and gs.dtype == torch.float32
        with torch.no_grad():                        # the forward is the inference call, bit for bit
            assert torch.equal(out, ops.nw_head_values(c.qd, c.sd, c.bank, c.vals, c.kind, c.ls(), **kw)), name
        close(gs, refs[name], f"gs {kind} {shape} {name}")
    # q, a clip scale, the values and the weights learning too: their gradients are the bits of the call where `s` does not
    # require grad, and gs the bits of the call where it learns alone
    kw = dict(c.variants["window and weights"][0])
    kw.pop("row_logw")
    got = []
    for s_grad in (False, True):
        v, a, ls = c.vd.clone().requires_grad_(True), c.ad.clone().requires_grad_(True), c.ls(grad=True)
        n0 = len(launches)
        _, gs2, gq = run(ops, c, c.gout, values=v, q_grad=True, s_grad=s_grad, row_logw=a, ls=ls, **kw)
        seen = launches[n0:]
        assert (seen.count(QUERY), seen.count(SUPPORT), seen.count(ROWS)) == (1, 1, int(s_grad)), seen
        got.append((gq, v.grad, a.grad, None if ls is None else ls.grad))
        assert (gs2 is None) == (not s_grad)
    for x, y in zip(*got):
        assert (x is None and y is None) or torch.equal(x, y)
    assert torch.equal(gs2, gs)


def test_log_outputs_under_a_kl_loss(O, ops, dev):
    c = case(O, ops, dev, SMALL, "euclidean")
    B, N, d, T = SMALL
    g = torch.Generator().manual_seed(8)
    soft = torch.softmax(torch.randn(N, T, generator=g), dim=1)
    target = torch.softmax(torch.randn(B, T, generator=g), dim=1)
    kw, rkw = c.variants["excluded single-row window"]
    ref = ref_gs(O, c.q, c.s, soft, "euclidean", {"kl": rkw},
                 lambda out: F.kl_div(torch.log(out + 1e-12), target.double(), reduction="batchmean"))["kl"]
    _, gs, _ = run(ops, c, values=soft.to(dev), log=True, loss=lambda out: F.kl_div(out, target.to(dev), reduction="batchmean"), **kw)
    close(gs, ref, "gs, log=True under a KL loss")


# ------------------------------------------------------------------------------------------------ 2. the class head
@pytest.mark.parametrize("kind", ("euclidean", "cosine"))
def test_one_hot_values_agree_with_the_class_head(O, ops, dev, kind):
    """One-hot values of the labels make the value head's output the class probabilities P; the class head returns
    log(P + 1e-12), so its upstream gradient g arrives at P as g exp(-out_class), over the classes that are present."""
    c = case(O, ops, dev, SMALL, kind)
    B, N, d, _ = SMALL
    syd = c.sy.to(dev)
    onehot = F.one_hot(c.sy, C16).float().to(dev)
    g = torch.randn(B, C16, generator=torch.Generator().manual_seed(4)).to(dev)
    for name in ("plain", "kept class window"):
        kw = c.variants[name][0]
        s = c.sd.requires_grad_(True)
        s.grad = None
        try:
            out_class = ops.nw_head_bank(c.qd, s, syd, C16, c.bank, kind, support_grad=True, **kw)
            out_class.backward(g)
            gs_class = s.grad.clone()
        finally:
            s.requires_grad_(False)
            s.grad = None
        oc = out_class.detach()
        # (an absent class is log(1e-12) up to fp32 rounding; the classes that are present here have P of the order 1 / 16)
        gv = torch.where(oc > math.log(1e-12) + 1e-3, g * torch.exp(-oc), torch.zeros_like(g))
        _, gs, _ = run(ops, c, gv, values=onehot, **kw)
        close(gs, gs_class, f"gs of one-hot values vs nw_head_bank(support_grad=True), {kind}, {name}")


# ------------------------------------------------------------------------------------------------ 3. exact zeros
@pytest.mark.parametrize("kind", ("euclidean", "clip"))
def test_rows_nobody_weighs_get_positive_zeros(O, ops, dev, kind):
    c = case(O, ops, dev, SMALL, kind)
    B, N, d, T = SMALL
    a = c.a.clone()
    a[64:128] = -INF                                          # a whole 64-row support tile at -inf
    ad = a.to(dev)
    off = a == -INF
    asked = torch.zeros(C16, dtype=torch.bool)
    asked[c.qy] = True
    unasked = ~asked[c.sy]                                    # rows no query's class window admits
    assert unasked.any() and not unasked.all()
    keep = c.variants["kept class window"][1]["keep"]
    win = c.variants["kept class window"][0]["row_window"]
    loss = lambda out: (out * c.gout.double()).sum()          # noqa: E731
    refs = ref_gs(O, c.q, c.s, c.v, kind, {"weights": dict(a=a), "window": dict(keep=keep), "both": dict(a=a, keep=keep)}, loss)
    for name, kw, dead in (("weights", dict(row_logw=ad), off), ("window", dict(row_window=win), unasked),
                           ("both", dict(row_window=win, row_logw=ad), off | unasked)):
        _, gs, _ = run(ops, c, c.gout, **kw)
        close(gs, refs[name], f"gs with rows nobody weighs, {kind}, {name}")
        assert int(dead.sum()) >= 64 and is_pos_zero(gs[dead.to(dev)]), name
        assert bool((refs[name][dead] == 0).all()) and float(gs[(~dead).to(dev)].abs().max()) > 0, name
    # a dead query (its class window holds rows at -inf alone) contributes nothing: the same gs without it, bit for bit ...
    assert not (keep[1] & ~off).any()
    _, gs_all, _ = run(ops, c, c.gout, row_window=win, row_logw=ad)
    lo2, hi2 = win[0].clone(), win[1].clone()
    hi2[1] = lo2[1]                                           # ... when its window is empty instead
    _, gs_empty, _ = run(ops, c, c.gout, row_window=(lo2, hi2), row_logw=ad)
    assert torch.equal(gs_all, gs_empty)
    # a batch of dead queries alone (empty kept windows): +0.0 everywhere
    out, gs, _ = run(ops, c, c.gout, row_window=(win[0], win[0]), row_logw=ad)
    assert is_pos_zero(gs) and bool((out == 0).all())


# ------------------------------------------------------------------------------------------------ 4. degenerate inputs
BIG = (64, 1024, 64, 5)


@pytest.mark.parametrize("kind", ("euclidean", "hypersphere_euclidean"))
def test_distance_derivative_takes_the_raw_score(O, ops, dev, kind):
    """a = +3 on a near row: with the weighted score in the distance's place 1 / D is off by far more than the bar."""
    c = case(O, ops, dev, BIG, kind)
    q0 = c.q.clone()
    q0[3] = c.s[100] + 0.05 * torch.randn(64, generator=torch.Generator().manual_seed(4))      # a near row
    logw = torch.zeros(BIG[1])
    logw[100] = 3.0
    ref = ref_gs(O, q0, c.s, c.v, kind, {"raw": dict(a=logw)}, lambda out: (out * c.gout.double()).sum())["raw"]
    _, gs, _ = run(ops, c, c.gout, q=q0, row_logw=logw.to(dev))
    close(gs, ref, f"gs with a = +3 on a near row {kind}")
    close(gs[100:101], ref[100:101], f"gs of the near row itself {kind}")


@pytest.mark.parametrize("kind", KINDS)
def test_an_all_zero_query_bank_row_and_gout_row(O, ops, dev, kind):
    c = case(O, ops, dev, BIG, kind)
    B, N, d, T = BIG
    z = N // 3
    q0, s0, gout = c.q.clone(), c.s.clone(), c.gout.clone()
    q0[B // 2] = 0.0
    s0[z] = 0.0
    gout[5] = 0.0
    sd = s0.to(dev)
    bank = ops.SplitBank(sd)
    ref = ref_gs(O, q0, s0, c.v, kind, {"zero": {}}, lambda out: (out * gout.double()).sum())["zero"]
    _, gs, _ = run(ops, c, gout, q=q0, sd=sd, bank=bank, values=ops.BankValues(c.vd, bank))
    close(gs, ref, f"gs zero query, zero row and zero gout row {kind}")
    # The other rows on their own scale.  The normalising kinds give the zero row a gradient of the order 1 / 1e-12 (so does
    # the reference), which is the scale of the comparison above; the workgroup's exponent follows it, and the 63 rows that
    # share its support tile keep only what lies within 2^-40 of it: they are left out here, as in
    # test_bank_support_grad_gpu.py.
    other = torch.ones(N, dtype=torch.bool)
    if kind in ("euclidean", "dotproduct"):
        other[z] = False
    else:
        other[z // 64 * 64:z // 64 * 64 + 64] = False
    close(gs[other.to(dev)], ref[other], f"gs of the other rows, zero query, zero row and zero gout row {kind}")


# ------------------------------------------------------------------------------------------------ 5. direct calls
def direct(c, dev, ops, gout, query_chunks=0, poison=None, window=None, exclude=False):
    """nw_bwd_values_bank_support_f32 called directly with a workspace of the caller's (poison: byte to fill it with) -> gs at
    the bank's (padded) width."""
    from nwhead_amd import _lib
    lib = _lib.load()
    B, N, _, T = c.shape
    Tp = T + (-T) % 32
    kid = ops.SCORE_KINDS[c.kind]
    q, d = ops._resolve_scores(c.bank, c.qd).q.contiguous(), c.bank.shape[1]
    rows = c.bank.rows if c.bank.rows is not None else c.sd
    ls = c.ls()
    with torch.no_grad():
        out, lse = ops.nw_head_values(c.qd, c.sd, c.bank, c.vals, c.kind, ls, row_window=window, exclude=exclude, return_lse=True)
    outp, g = F.pad(out, (0, Tp - T)).contiguous(), F.pad(gout.to(dev), (0, Tp - T)).contiguous()
    lo, hi = (t.to(torch.int32).contiguous() for t in window) if window is not None else (None, None)
    need = lib.nw_bwd_values_bank_support_workspace_bytes(B, N, d, Tp, query_chunks)
    assert 0 < need
    ws = torch.full((need,), 0 if poison is None else poison, dtype=torch.uint8, device=dev)
    gs = torch.empty(N, d, device=dev)
    _lib.check(lib.nw_bwd_values_bank_support_f32(q.data_ptr(), rows.data_ptr(), c.bank.split.data_ptr(), c.bank.scale.data_ptr(),
                                                  c.bank.norm2.data_ptr(), c.vals.split.data_ptr(), c.vals.scale.data_ptr(), None,
                                                  None if lo is None else lo.data_ptr(), None if hi is None else hi.data_ptr(),
                                                  int(exclude), lse.data_ptr(), outp.data_ptr(), g.data_ptr(), gs.data_ptr(),
                                                  ws.data_ptr(), need, B, N, d, Tp, kid, None if ls is None else ls.data_ptr(),
                                                  query_chunks, None), "nw_bwd_values_bank_support_f32")
    torch.cuda.synchronize()
    return gs


WIDE = (300, 200, 64, 5)            # five query tiles over four support tiles


@pytest.mark.parametrize("shape", [PADDED, WIDE], ids=lambda s: "x".join(map(str, s)))
def test_query_chunks_are_deterministic_and_within_the_bar(O, ops, dev, shape):
    c = case(O, ops, dev, shape, "euclidean")
    ref = c.parity_refs()["plain"]
    n_qtiles = -(-shape[0] // 64)
    for qc in sorted({1, 2, 3, n_qtiles}):
        gs = direct(c, dev, ops, c.gout, qc)
        close(gs[:, :shape[2]], ref, f"gs query_chunks={qc} {shape}")
        assert is_pos_zero(gs[:, shape[2]:])                                    # the zero columns of a padded bank
        assert torch.equal(gs, direct(c, dev, ops, c.gout, qc)), qc             # two calls: identical bits


@pytest.mark.parametrize("kind", ("euclidean", "clip"))
def test_poisoned_workspace_changes_nothing(O, ops, dev, kind):
    c = case(O, ops, dev, PADDED, kind)
    for qc in (0, 1, 2):
        a, b = direct(c, dev, ops, c.gout, qc), direct(c, dev, ops, c.gout, qc, poison=0xFF)
        assert torch.isfinite(b).all() and torch.equal(a, b)
    lo = torch.arange(PADDED[0], device=dev) % 100
    win = (lo, lo + 150)
    a, b = direct(c, dev, ops, c.gout, 2, window=win), direct(c, dev, ops, c.gout, 2, poison=0xFF, window=win)
    assert torch.isfinite(b).all() and torch.equal(a, b)


@pytest.mark.parametrize("kind", ("euclidean", "cosine"))
def test_gout_times_a_power_of_two_scales_gs_exactly(O, ops, dev, kind):
    c = case(O, ops, dev, PADDED, kind)
    base = direct(c, dev, ops, c.gout, 2)
    assert float(base.abs().max()) > 0
    for k in (-20, -3, 7, 20):
        assert torch.equal(direct(c, dev, ops, c.gout * 2.0 ** k, 2), base * 2.0 ** k), k


# ------------------------------------------------------------------------------------------------ 6. memory
def test_no_score_matrix_is_allocated(O, ops, dev):
    B, N, d, T = 256, 32768, 64, 32
    g = torch.Generator().manual_seed(1)
    s = torch.randn(N, d, generator=g).to(dev)
    q = torch.randn(B, d, generator=g).to(dev)
    v = torch.randn(N, T, generator=g).to(dev)
    t = torch.randn(B, T, generator=g).to(dev)
    bank = ops.SplitBank(s)
    vals = ops.BankValues(v, bank)
    matrix = B * N * 4

    def peak(fn):
        # the forward's scratch and the backward's workspace are process-wide buffers that are only ever grown: they are
        # warmed by a first step and are not part of what a later step allocates; gs itself is the result
        for _ in range(2):
            s.grad = None
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(dev)
            before = torch.cuda.memory_allocated(dev)
            F.mse_loss(fn(s.requires_grad_(True)), t).backward()
            torch.cuda.synchronize()
            used = torch.cuda.max_memory_allocated(dev) - before
        grad = s.grad
        s.requires_grad_(False)
        s.grad = None
        return used - N * d * 4, grad

    fused, g1 = peak(lambda sp: ops.nw_head_values_bank(q, sp, bank, vals, support_grad=True))
    composed, g2 = peak(lambda sp: ops._values_head_matrix(q, sp, bank, v, "euclidean", None, None, None, None, False))
    print(f"MEM nw_head_values_bank(support_grad=True) {fused} bytes beyond gs, the matrix composition {composed} bytes, "
          f"one score matrix {matrix} bytes")
    assert fused < matrix
    assert composed > matrix                                 # the test can see the difference
    close(g1, g2, "gs at 256 x 32768 x 64 under mse_loss against the matrix composition")


# ------------------------------------------------------------------------------------------------ 7. the matrix route
def test_matrix_routes(O, ops, dev, launches):
    c = case(O, ops, dev, SMALL, "euclidean")
    B, N, d, T = SMALL
    refs = c.parity_refs()
    fp16 = ops.SplitBank(c.sd, precision="fp16")
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(3))
    unsorted = ops.SplitBank(c.sd, labels=c.sy[perm].to(dev))          # (only the bank's route depends on the labels)
    assert unsorted.sorted_rows is not None
    for name, bank in (("fp16 bank", fp16), ("unsorted labels", unsorted)):
        for variant in ("plain", "window and weights"):
            del launches[:]
            _, gs, gq = run(ops, c, c.gout, bank=bank, values=ops.BankValues(c.vd, bank), q_grad=True, **c.variants[variant][0])
            assert ROWS not in launches and QUERY not in launches and SUPPORT not in launches, (name, launches)
            close(gs, refs[variant], f"gs matrix route, {name}, {variant}")
            assert gq is not None and bool(torch.isfinite(gq).all())
    # N = 20, below the tile kernels
    N2 = 20
    s2, v2 = c.s[:N2].contiguous(), c.v[:N2].contiguous()
    a2 = torch.tensor(PATTERN)[torch.arange(N2) % 7].clone()
    lo2, hi2 = torch.arange(B) % N2, torch.arange(B) % N2 + 1 + (torch.arange(B) % 3)
    ref2 = ref_gs(O, c.q, s2, v2, "euclidean", {"plain": {}, "both": dict(a=a2, keep=_admitted(N2, lo2, hi2, False))},
                  lambda out: (out * c.gout.double()).sum())
    s2d = s2.to(dev).requires_grad_(True)
    bank2 = ops.SplitBank(s2d)
    for name, kw in (("plain", {}), ("both", dict(row_window=(lo2.to(dev), hi2.to(dev)), row_logw=a2.to(dev)))):
        s2d.grad = None
        del launches[:]
        ops.nw_head_values_bank(c.qd, s2d, bank2, v2.to(dev), support_grad=True, **kw).backward(c.gout.to(dev))
        assert ROWS not in launches and "nw_fwd_values_f32" not in launches, launches
        close(s2d.grad, ref2[name], f"gs matrix route, N = 20, {name}")


# ------------------------------------------------------------------------------------------------ 8. refusals
def test_default_keyword_still_refuses_a_support_that_requires_grad(ops, dev):
    s = torch.randn(100, 64, device=dev)
    bank = ops.SplitBank(s)
    v = torch.randn(100, 3, device=dev)
    with pytest.raises(ValueError, match="the bank is a constant here and `s` requires grad"):
        ops.nw_head_values_bank(torch.randn(4, 64, device=dev), s.requires_grad_(True), bank, v)


def test_a_backward_after_refresh_is_refused(ops, dev):
    s = torch.randn(200, 64, device=dev).requires_grad_(True)
    bank = ops.SplitBank(s)
    out = ops.nw_head_values_bank(torch.randn(8, 64, device=dev), s, bank, torch.randn(200, 3, device=dev), support_grad=True)
    bank.refresh(s)
    with pytest.raises(RuntimeError, match="the bank was written"):
        out.sum().backward()


# ------------------------------------------------------------------------------------------------ 9. NWNet
class _DS(torch.utils.data.Dataset):
    def __init__(self, data, targets, C):
        self.data, self.targets, self.num_classes = data, list(targets), C

    def __len__(self):
        return len(self.targets)

    def __getitem__(self, i):
        return self.data[i], self.targets[i]


def test_nwnet_learnable_keys_and_values(O, dev):
    from nwhead_amd import ops
    from nwhead_amd.nwhead.nw import NWNet
    g = torch.Generator().manual_seed(5)
    C, n, din, d, T = 6, 40, 48, 64, 3
    data = torch.randn(C * n, din, generator=g)
    targets = (torch.arange(C * n) % C).tolist()
    feat = nn.Linear(din, d)
    with torch.no_grad():
        feat.weight.copy_(torch.randn(d, din, generator=g) * din ** -0.5)
        feat.bias.copy_(torch.randn(d, generator=g) * 0.1)
    net = NWNet(feat, C, support_dataset=_DS(data, targets, C), n_shot=2, n_way=C, n_shot_full=n, device="cuda:0").to(dev)
    net.eval()
    np.random.seed(11)
    net.precompute()
    N = net.full_feat.shape[0]
    v0 = torch.randn(N, T, generator=g)
    net.set_support_values(v0, learnable=True)
    net.set_bank_learnable()
    names = dict(net.named_parameters())
    assert "support_bank" in names and "support_targets" in names
    B = 24
    x = torch.randn(B, din, generator=g)
    rows = torch.randint(0, N, (B,), generator=g)
    rows[::4] = -1
    gout = torch.randn(B, T, generator=g)
    lo = rows.clamp(min=0)
    keep = _admitted(N, lo, torch.where(rows < 0, lo, lo + 1), True)
    W, b = feat.weight.detach().cpu().double(), feat.bias.detach().cpu().double()
    rs = ref_gs(O, x.double() @ W.t() + b, net.full_feat.detach().cpu(), v0, "euclidean", {"loo": dict(keep=keep)},
                lambda out: (out * gout.double()).sum())["loo"]
    net.zero_grad()
    cache, ptr = net.full_cache, net.full_cache.split.data_ptr()
    out = net.forward_values(x.to(dev), leave_out=rows.to(dev))
    out.backward(gout.to(dev))
    close(net.support_bank.grad, rs, "support_bank.grad, forward_values with leave_out")
    assert net.support_targets.grad is not None and float(net.support_targets.grad.abs().max()) > 0
    assert feat.weight.grad is not None and feat.bias.grad is not None
    # an optimizer step on the rows: the next calls read the bank re-prepared in place, bit for bit a freshly built one
    torch.optim.SGD([net.support_bank], lr=0.5).step()
    with torch.no_grad():
        again = net.forward_values(x.to(dev), leave_out=rows.to(dev))
        assert net.full_cache is cache and cache.split.data_ptr() == ptr and cache.matches(net.full_feat)
        fresh = ops.SplitBank(net.full_feat.detach().clone(), labels=net.full_y)
        assert torch.equal(cache.split, fresh.split) and torch.equal(cache.norm2, fresh.norm2) and torch.equal(cache.scale, fresh.scale)
        assert bool(torch.isfinite(again).all()) and not torch.equal(again, out.detach())
    # learnable weights beside the rows and the values
    net.set_support_weights(torch.zeros(N, device=dev), learnable=True)
    net.zero_grad()
    net.forward_values(x.to(dev), leave_out=rows.to(dev), weights_grad=True).backward(gout.to(dev))
    assert net.support_logw.grad is not None and net.support_bank.grad is not None and net.support_targets.grad is not None
