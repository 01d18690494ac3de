"""Learnable support weights: the gradient of the weighted head w.r.t. ``row_logw`` (nw_bwd_query_logw_f32 through
ops.nw_head_bank(row_logw=a) with a.requires_grad, and NWNet.set_support_weights(learnable=True)).

ga_j = sum_b W_bj (dP_b[y_j] - t_b), W_bj = exp(score_bj + a_j - lse_b): the column sums over the queries of what the query
gradient contracts with the bank rows, taken in the same kernel (bwd_query.hip, GA), no (B, N) buffer.

Reference: fp64 torch on the CPU, autograd through log(softmax(score + a over the admitted rows) @ one_hot + 1e-12) -- _head_f64
of test_head_weighted_gpu.py, restated here with the weights in the graph.  Standard weights of that file: a_j by j mod 7 =
{0, ln 2, -3.5, -inf, 0, 1.25, -0.5} and one whole class at -inf.
Bar: the project's gradient bar, rtol = atol = 1e-4 on values divided by max(|ref|.max(), 1e-3); logit_scale.grad rtol 1e-4,
atol 1e-6.  ga is a signed sum over the queries: should a shape miss the bar through cancellation, the allowance is twice
the error of the fp32 matrix route (ops.nw_scores + a + ops.nw_aggregate with autograd) at the same inputs against the same
reference (_ga_close).  No shape of this file needs it (one MI355X): the normalised error of ga is 2.8e-7 .. 1.1e-6 in
every case but the kept class windows at (37, 4100, 96), 2.6e-5 (one or two queries per row), so the matrix route's error
was never taken; logit_scale.grad sits at 9.5e-5 relative with gq (nw_bwd_query_weighted_f32's own bits) and 1.03e-4
without, inside rtol 1e-4 + atol 1e-6.
Every direct call runs on a workspace filled with 0xFF and writes into a glogw filled with NaN beforehand."""
import math

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import ws_poison

pytestmark = pytest.mark.gpu

NEG_INF = float("-inf")
LS0 = float(np.log(1 / 0.07))
KINDS = ("euclidean", "hypersphere_euclidean", "cosine", "dotproduct", "clip")
SHAPES = [(37, 4100, 96), (130, 1000, 64), (256, 2048, 512)]
C16 = 16
PATTERN = (0.0, math.log(2.0), -3.5, NEG_INF, 0.0, 1.25, -0.5)
DEAD_CLASS = 3
FWD, BWD_W, BWD_A = "nw_fwd_weighted_f32", "nw_bwd_query_weighted_f32", "nw_bwd_query_logw_f32"
SPIED = (FWD, BWD_W, BWD_A, "nw_fwd_window_f32", "nw_bwd_query_f32", "nw_fwd_f32", "nw_scores_f32", "nw_aggregate_f32")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "run with -m gpu on the MI355X box"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from nwhead_amd import ops as o
    return o


@pytest.fixture(autouse=True)
def _no_split_always(monkeypatch):
    monkeypatch.delenv("NW_SPLIT_ALWAYS", raising=False)


@pytest.fixture
def launches(monkeypatch):
    """Records the name of every head entry point that is launched, with gq's pointer for the weights' entry."""
    from nwhead_amd import _lib
    lib = _lib.load()
    calls = []

    class Spy:
        def __getattr__(self, name):
            real = getattr(lib, name)
            if name == BWD_A:
                return lambda *a: (calls.append(name + ("" if a[12] else "(gq=NULL)")), real(*a))[1]
            if name in SPIED:
                return lambda *a: (calls.append(name), real(*a))[1]
            return real

    monkeypatch.setattr(_lib, "_lib", Spy())
    return calls


# ------------------------------------------------------------------------------------------------ data and reference
def _std_logw(sy, dead_class=DEAD_CLASS):
    a = torch.tensor(PATTERN, dtype=torch.float32)[torch.arange(len(sy)) % 7].clone()
    if dead_class is not None:
        a[sy == dead_class] = NEG_INF
    return a


def _class_windows(sy, B, C=C16, seed=11):
    qy = torch.randint(0, C, (B,), generator=torch.Generator().manual_seed(seed))
    return torch.searchsorted(sy, qy), torch.searchsorted(sy, qy, right=True), qy


def _admitted(N, lo, hi, exclude):
    cols = torch.arange(N)
    inside = (cols >= lo.clamp(0, N)[:, None]) & (cols < hi.clamp(0, N)[:, None])
    return ~inside if exclude else inside


def _scores_f64(q, s, kind, ls=None):
    """fp64 scores of constant queries (no gradient goes to them here)."""
    q, s = q.double(), s.double()
    if kind in ("hypersphere_euclidean", "cosine", "clip"):
        q = q / q.norm(dim=-1, keepdim=True).clamp_min(1e-12)
        s = s / s.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    if kind in ("euclidean", "hypersphere_euclidean"):
        return -torch.cdist(q, s, compute_mode="donot_use_mm_for_euclid_dist")
    dot = q @ s.T
    if kind == "clip":
        return (ls.exp() if torch.is_tensor(ls) else math.exp(float(ls))) * dot
    return dot


def _head_f64(q, s, sy, C, a, window=None, exclude=False, kind="euclidean", ls=None):
    """-> (log-probs, number of dead queries) in fp64 on the CPU; ``a`` (fp64, maybe in a graph) enters through its finite
    entries, a row at -inf is not admitted."""
    N = s.shape[0]
    finite = a.detach() > NEG_INF
    admit = finite[None].expand(q.shape[0], N)
    if window is not None:
        admit = admit & _admitted(N, window[0], window[1], exclude)
    sc = _scores_f64(q, s, kind, ls) + torch.where(finite, a, torch.zeros_like(a)).double()[None]
    sc = sc.masked_fill(~admit, NEG_INF)
    live = admit.any(dim=1, keepdim=True)
    w = torch.where(live, torch.softmax(torch.where(live, sc, torch.zeros_like(sc)), dim=-1), torch.zeros_like(sc))
    return torch.log(w @ F.one_hot(sy, C).double() + 1e-12), int((~live).sum())


class Case:
    """Inputs on the CPU and the device, the class-sorted bank prepared once, references memoised."""

    def __init__(self, ops, dev, B, N, d, kind="euclidean", C=C16):
        g = torch.Generator().manual_seed(B * 7919 + N * 31 + d)
        self.q0, self.s0 = torch.randn(B, d, generator=g), torch.randn(N, d, generator=g)
        if kind == "dotproduct":
            self.q0, self.s0 = self.q0 * d ** -0.25, self.s0 * d ** -0.25
        self.sy0 = (torch.arange(N) % C).sort().values
        self.q, self.s, self.sy = self.q0.to(dev), self.s0.to(dev), self.sy0.to(dev)
        self.bank = ops.SplitBank(self.s, labels=self.sy)
        self.B, self.N, self.d, self.C, self.kind = B, N, d, C, kind
        self.gout = torch.randn(B, C, generator=torch.Generator().manual_seed(7))
        self.a = _std_logw(self.sy0)
        self.memo = {}

    def ls(self, dev=None, grad=True):
        if self.kind != "clip":
            return None
        return torch.tensor(LS0, dtype=torch.float64 if dev is None else torch.float32, device=dev, requires_grad=grad)

    def ref(self, tag, a, window=None, exclude=False, q0=None, gout=None):
        """(ga, glogit_scale or None, dead queries, out) in fp64."""
        if tag not in self.memo:
            a64 = a.double().requires_grad_(True)
            ls = self.ls()
            out, dead = _head_f64(self.q0 if q0 is None else q0, self.s0, self.sy0, self.C, a64, window, exclude, self.kind, ls)
            gr = torch.autograd.grad((out * (self.gout if gout is None else gout).double()).sum(), (a64,) + ((ls,) if ls is not None else ()))
            self.memo[tag] = (gr[0], gr[1] if ls is not None else None, dead, out.detach())
        return self.memo[tag]


_CASES = {}


def _case(ops, dev, shape, kind="euclidean"):
    if (shape, kind) not in _CASES:
        _CASES[(shape, kind)] = Case(ops, dev, *shape, kind)
    return _CASES[(shape, kind)]


@pytest.fixture(scope="module", autouse=True)
def _drop_cases():
    yield
    _CASES.clear()


def _norm_err(got, ref):
    got, ref = got.detach().cpu().double(), ref.detach().double()
    return float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-3)


def _gclose(got, ref, what, ls=False):
    got, ref = got.detach().cpu().double().numpy(), ref.detach().double().numpy()
    assert np.isfinite(got).all(), what
    if ls:
        print(f"ERR {float(abs(got - ref)) / max(float(abs(ref)), 1e-30):.3e} (relative) {what}")
        np.testing.assert_allclose(got, ref, rtol=1e-4, atol=1e-6, err_msg=what)
        return
    scale = max(float(np.abs(ref).max()), 1e-3)
    print(f"ERR {float(np.abs(got - ref).max()) / scale:.3e} {what}")
    np.testing.assert_allclose(got / scale, ref / scale, rtol=1e-4, atol=1e-4, err_msg=what)


def _matrix_ga(ops, dev, c, a, gout=None):
    """ga of the fp32 route through the score matrix: nw_scores + a + nw_aggregate with autograd (no window)."""
    ad = a.to(dev).requires_grad_(True)
    out = ops.nw_aggregate(ops.nw_scores(c.q, c.s, c.kind, c.ls(dev, False), support_cache=c.bank) + ad, c.sy, c.C)
    out.backward((c.gout if gout is None else gout).to(dev))
    return ad.grad


def _ga_close(ops, dev, c, got, ref, what, a=None):
    """The bar; on a miss (cancellation in the signed sum over the queries) twice the matrix route's own error, where that
    route exists (no window)."""
    assert bool(torch.isfinite(got).all()), what
    err = _norm_err(got, ref)
    print(f"ERR {err:.3e} ga {what}")
    try:
        _gclose(got, ref, "ga " + what)
    except AssertionError:
        if a is None:
            raise
        merr = _norm_err(_matrix_ga(ops, dev, c, a), ref)
        print(f"ERR {merr:.3e} ga of the matrix route {what}")
        assert err <= 2 * merr, (what, err, merr)


def _direct(ops, dev, c, a, window=None, exclude=False, row_chunks=0, want_gq=True, q0=None, entry=BWD_A, gout=None):
    """The forward through ops, then nw_bwd_query_logw_f32 (or nw_bwd_query_weighted_f32) called directly on a poisoned
    workspace of the caller's -> (ga, gq, glogit_scale); ga starts as NaN, gq as NaN."""
    from nwhead_amd import _lib
    lib = _lib.load()
    B, N, d, C = c.B, c.N, c.d, c.C
    kid = ops.SCORE_KINDS[c.kind]
    q = c.q if q0 is None else q0.to(dev)
    ls = c.ls(dev, False)
    win = None if window is None else tuple(t.to(dev).to(torch.int32).contiguous() for t in window)
    ad = a.to(dev)
    with torch.no_grad():
        out, lse = ops.nw_head_window(q, c.s, c.sy, C, c.bank, win, exclude, c.kind, ls, return_lse=True, row_logw=ad)
    if entry == BWD_A:
        need = lib.nw_bwd_logw_workspace_bytes(B, N, d, C, row_chunks, int(want_gq))
    else:
        need = lib.nw_bwd_query_workspace_bytes(B, N, d, C, row_chunks)
    assert need > 0
    ws = ws_poison.poisoned_workspace(need, dev)
    nan = float("nan")
    gq = torch.full((B, d), nan, device=dev) if want_gq else None
    ga, gls = torch.full((N,), nan, device=dev), torch.full((), nan, device=dev)
    g = (c.gout if gout is None else gout).to(dev).contiguous()
    lo, hi = (None, None) if win is None else (win[0].data_ptr(), win[1].data_ptr())
    bank = (c.bank.split.data_ptr(), c.bank.scale.data_ptr(), c.bank.norm2.data_ptr(), c.sy.data_ptr())
    head = (q.data_ptr(), *bank, ad.data_ptr(), lo, hi, int(exclude), lse.data_ptr(), out.data_ptr(), g.data_ptr(),
            None if gq is None else gq.data_ptr())
    tail = (gls.data_ptr(), ws.data_ptr(), need, B, N, d, C, kid, None if ls is None else ls.data_ptr(), row_chunks, None)
    if entry == BWD_A:
        _lib.check(lib.nw_bwd_query_logw_f32(*head, ga.data_ptr(), *tail), BWD_A)
    else:
        _lib.check(lib.nw_bwd_query_weighted_f32(*head, *tail), BWD_W)
    torch.cuda.synchronize()
    return ga, gq, gls


def _positive_zero(x):
    """Every element is +0.0: equal to zero with the sign bit clear."""
    return bool((x == 0).all()) and not bool(torch.signbit(x).any())


# ------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("B,N,d,kind", [(*SHAPES[0], k) for k in KINDS] + [(*s, k) for s in SHAPES[1:] for k in ("euclidean", "cosine")])
def test_parity(ops, dev, launches, B, N, d, kind):
    """(37, 4100, 96): B below a query tile, N ragged against 64; (130, 1000, 64): three query tiles (the reduction over
    them), one slab; (256, 2048, 512): several slabs, of which only slab 0 may write.  Through autograd (weights only and
    with the queries) and through the C entry, both variants."""
    c = _case(ops, dev, (B, N, d), kind)
    rga, rls, dead, _ = c.ref("std", c.a)
    assert dead == 0
    ls = c.ls(dev)
    a = c.a.to(dev).requires_grad_(True)
    ops.nw_head_bank(c.q, c.s, c.sy, c.C, c.bank, kind, ls, row_logw=a).backward(c.gout.to(dev))
    assert launches == [FWD, BWD_A + ("" if kind == "clip" else "(gq=NULL)")]
    _ga_close(ops, dev, c, a.grad, rga, f"{kind} {(B, N, d)} autograd, weights only", c.a)
    assert _positive_zero(a.grad[c.a.to(dev) == NEG_INF])
    if kind == "clip":
        _gclose(ls.grad, rls, "logit_scale.grad clip, autograd", ls=True)
    for want_gq in (False, True):
        ga, gq, gls = _direct(ops, dev, c, c.a, want_gq=want_gq)
        _ga_close(ops, dev, c, ga, rga, f"{kind} {(B, N, d)} direct want_gq={want_gq}", c.a)
        if kind == "clip":
            _gclose(gls, rls, f"logit_scale.grad clip, direct want_gq={want_gq}", ls=True)
        else:
            assert float(gls) == 0.0
        assert gq is None or bool(torch.isfinite(gq).all())
        assert torch.equal(ga, a.grad)          # row_chunks = 0 here as in autograd; and both variants give the same bits


# ------------------------------------------------------------------------------------------------ 2. chunks
@pytest.mark.parametrize("kind", ("euclidean", "clip"))
@pytest.mark.parametrize("shape", SHAPES[:2], ids=lambda s: "x".join(map(str, s)))
def test_chunks_do_not_enter_the_sum(ops, dev, shape, kind):
    """row_chunks in {1, 3, the tile count} through the C entry, each twice, on poisoned workspaces: ga identical bits
    throughout (chunks own disjoint rows), in both variants."""
    c = _case(ops, dev, shape, kind)
    tiles = (c.N + 63) // 64
    lo, hi, _ = _class_windows(c.sy0, c.B)
    for win, exclude in ((None, False), ((lo, hi), True)):
        first = None
        for rc in (1, 3, tiles):
            for want_gq in (False, True):
                one = _direct(ops, dev, c, c.a, win, exclude, rc, want_gq)
                two = _direct(ops, dev, c, c.a, win, exclude, rc, want_gq)
                assert bool(torch.isfinite(one[0]).all()) and torch.equal(one[0], two[0]), (rc, want_gq)
                if want_gq:
                    assert torch.equal(one[1], two[1]) and torch.equal(one[2], two[2])
                first = one[0] if first is None else first
                assert torch.equal(one[0], first), (rc, want_gq)
        rga = c.ref("std" if win is None else "excl", c.a, win, exclude)[0]
        _ga_close(ops, dev, c, first, rga, f"{kind} {shape} chunks, window={win is not None}")


# ------------------------------------------------------------------------------------------------ 3. bit identity between the variants
@pytest.mark.parametrize("shape,kind", [(SHAPES[0], k) for k in KINDS] + [(SHAPES[2], k) for k in ("euclidean", "cosine", "clip")],
                         ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_variants_agree_bit_for_bit(ops, dev, shape, kind):
    """The weights-only ga equals the gq + ga call's ga; that call's gq and glogit_scale equal nw_bwd_query_weighted_f32's.
    All five kinds at the small shape, three at the one with several slabs."""
    c = _case(ops, dev, shape, kind)
    lo, hi, _ = _class_windows(c.sy0, c.B)
    for win, exclude in ((None, False), ((lo, hi), False), ((lo, hi), True)):
        for rc in (0, 3):
            ga2, _, gls2 = _direct(ops, dev, c, c.a, win, exclude, rc, want_gq=False)
            ga1, gq1, gls1 = _direct(ops, dev, c, c.a, win, exclude, rc, want_gq=True)
            _, gq0, gls0 = _direct(ops, dev, c, c.a, win, exclude, rc, entry=BWD_W)
            assert torch.equal(ga1, ga2), (win is not None, exclude, rc)
            assert torch.equal(gq1, gq0) and torch.equal(gls1, gls0), (win is not None, exclude, rc)
            assert bool(torch.isfinite(gq1).all()) and bool(torch.isfinite(gls2))
            if kind == "clip":
                _gclose(gls2, gls0.cpu(), "glogit_scale of the weights-only variant against the weighted backward's", ls=True)


# ------------------------------------------------------------------------------------------------ 4. exact zeros, windows, dead queries
def test_exact_zeros_and_windows(ops, dev):
    B, N, d = SHAPES[0]
    c = _case(ops, dev, (B, N, d))
    a_dev = c.a.to(dev)
    # kept class windows: a query of the class whose rows are all at -inf is dead; rows of classes nobody asks for, rows at
    # -inf and the rows of the dead class: exactly +0.0
    lo, hi, qy = _class_windows(c.sy0, B)
    rga, _, dead, _ = c.ref("kept", c.a, (lo, hi), False)
    assert dead == int((qy == DEAD_CLASS).sum()) and dead > 0
    asked = torch.isin(c.sy0, qy)
    assert bool((~asked).any())
    for want_gq in (False, True):
        ga, gq, _ = _direct(ops, dev, c, c.a, (lo, hi), False, 3, want_gq)
        _gclose(ga, rga, f"ga kept class windows want_gq={want_gq}")
        assert _positive_zero(ga[(~asked).to(dev)]) and _positive_zero(ga[a_dev == NEG_INF])
        assert float(ga.abs().max()) > 0
        if want_gq:
            assert bool((gq[(qy == DEAD_CLASS).to(dev)] == 0).all())
    # leave-one-out of the bank's own rows: every query is a bank row and leaves itself out.  (A copy that is NOT left out
    # sits at distance 0, which the matmul form of the scores resolves to ~1e-3 only -- a property of the forward, see
    # test_head_weighted_gpu.py -- and its weight W ~ 1 carries that into ga: 2.2e-3 measured; such pairs are not this test's.)
    rows = (torch.arange(B) * (N // B)) + 1
    q0 = c.s0[rows].clone()
    wlo, whi = rows.clone(), rows + 1
    rga = c.ref("loo", c.a, (wlo, whi), True, q0)[0]
    for want_gq in (False, True):
        ga, _, _ = _direct(ops, dev, c, c.a, (wlo, whi), True, 0, want_gq, q0)
        _gclose(ga, rga, f"ga leave-one-out want_gq={want_gq}")
        assert _positive_zero(ga[a_dev == NEG_INF])
    # an all-empty window batch: every query dead, ga is +0.0 everywhere, no NaN
    empty = (torch.full((B,), 7), torch.full((B,), 7))
    for want_gq in (False, True):
        ga, gq, gls = _direct(ops, dev, c, c.a, empty, False, 3, want_gq)
        assert _positive_zero(ga) and float(gls) == 0.0 and (gq is None or bool((gq == 0).all()))
    # every admitted row at -inf for some queries (a whole 16-query wave and strays): they contribute nothing
    a = _std_logw(c.sy0, dead_class=None)
    a[255:300] = NEG_INF
    klo, khi = torch.zeros(B, dtype=torch.int64), torch.full((B,), N)
    dead_q = list(range(16, 32)) + [0, 36]
    klo[dead_q], khi[dead_q] = 260, 290
    rga, _, dead, _ = c.ref("dead", a, (klo, khi), False)
    assert dead == len(dead_q)
    live = torch.ones(B, dtype=torch.bool)
    live[dead_q] = False
    for want_gq in (False, True):
        ga, _, _ = _direct(ops, dev, c, a, (klo, khi), False, 0, want_gq)
        _gclose(ga, rga, f"ga with dead queries want_gq={want_gq}")
        assert _positive_zero(ga[255:300])
    # ... the same ga as the batch of the live queries alone gives, to the bar (the dead ones add exact zeros)
    only = Case(ops, dev, int(live.sum()), N, d)
    only.q0, only.q, only.s0, only.s, only.sy0, only.sy, only.bank = c.q0[live], c.q[live.to(dev)].contiguous(), c.s0, c.s, c.sy0, c.sy, c.bank
    ga_live, _, _ = _direct(ops, dev, only, a, (klo[live], khi[live]), False, 0, False, gout=c.gout[live])
    _gclose(ga, ga_live.cpu(), "dead queries add nothing")
    # every weight at -inf
    ga, _, _ = _direct(ops, dev, c, torch.full((N,), NEG_INF), want_gq=False)
    assert _positive_zero(ga)


# ------------------------------------------------------------------------------------------------ 5. shift invariance
@pytest.mark.parametrize("kind", ("euclidean", "cosine"))
def test_shift_invariance(ops, dev, kind):
    """softmax(score + a) does not see a constant added to every finite a: sum(ga) ~ 0 (bound 1e-4 sum |ga|, with no class
    probability at the 1e-12 floor: finite weights, every class populated, log-probabilities far above log 1e-12) and ga
    itself is unchanged within the bar."""
    B, N, d = SHAPES[1]
    c = _case(ops, dev, (B, N, d), kind)
    a = _std_logw(c.sy0, dead_class=None)
    a[a == NEG_INF] = -1.0
    rga, _, _, out = c.ref("finite", a)
    assert float(out.min()) > math.log(1e-9)
    ga, _, _ = _direct(ops, dev, c, a, want_gq=False)
    _gclose(ga, rga, f"ga finite weights {kind}")
    total, mass = float(ga.double().sum()), float(ga.double().abs().sum())
    print(f"SUM {total:.3e} of {mass:.3e}")
    assert abs(total) <= 1e-4 * mass
    ga_shift, _, _ = _direct(ops, dev, c, a + 2.5, want_gq=False)
    _gclose(ga_shift, rga, f"ga after a += 2.5 {kind}")
    # with -inf rows: the finite ones shifted
    ga0, _, _ = _direct(ops, dev, c, c.a, want_gq=True)
    ga1, _, _ = _direct(ops, dev, c, torch.where(c.a > NEG_INF, c.a - 1.75, c.a), want_gq=True)
    _gclose(ga1, ga0.cpu(), f"ga after finite a -= 1.75 {kind}")


# ------------------------------------------------------------------------------------------------ 6. autograd
def test_autograd_leaf_with_queries(ops, dev, launches):
    """q and a both require grad: one forward and one backward launch set; gq is the weighted backward's bit for bit."""
    c = _case(ops, dev, SHAPES[0])
    q = c.q.clone().requires_grad_(True)
    a = c.a.to(dev).requires_grad_(True)
    out = ops.nw_head_bank(q, c.s, c.sy, c.C, c.bank, row_logw=a)
    out.backward(c.gout.to(dev))
    assert launches == [FWD, BWD_A]
    assert a.grad is not None and a.grad.dtype == torch.float32 and a.grad.shape == (c.N,)
    _gclose(a.grad, c.ref("std", c.a)[0], "a.grad with q.grad")
    _, gq0, _ = _direct(ops, dev, c, c.a, entry=BWD_W)
    assert torch.equal(q.grad, gq0)
    # the forward is the inference call's, bit for bit, and a constant a keeps the old entry
    with torch.no_grad():
        assert torch.equal(out.detach(), ops.nw_head(c.q, c.s, c.sy, c.C, support_cache=c.bank, row_logw=c.a.to(dev)))
    del launches[:]
    q2 = c.q.clone().requires_grad_(True)
    ops.nw_head_bank(q2, c.s, c.sy, c.C, c.bank, row_logw=c.a.to(dev)).backward(c.gout.to(dev))
    assert launches == [FWD, BWD_W] and torch.equal(q2.grad, q.grad)


def test_autograd_only_the_weights(ops, dev, launches):
    """Only a requires grad: the gq-free variant; q gets no gradient; under no_grad nothing is recorded."""
    c = _case(ops, dev, SHAPES[1])
    a = c.a.to(dev).requires_grad_(True)
    out = ops.nw_head_bank(c.q, c.s, c.sy, c.C, c.bank, row_logw=a)
    assert out.requires_grad
    out.backward(c.gout.to(dev))
    assert launches == [FWD, BWD_A + "(gq=NULL)"]
    _gclose(a.grad, c.ref("std", c.a)[0], "a.grad, weights only")
    with torch.no_grad():
        assert not ops.nw_head_bank(c.q, c.s, c.sy, c.C, c.bank, row_logw=a).requires_grad
    # with a window (leave-one-out of the bank's own rows is not needed for that: class windows, excluded)
    lo, hi, _ = _class_windows(c.sy0, c.B)
    a2 = c.a.to(dev).requires_grad_(True)
    ops.nw_head_bank(c.q, c.s, c.sy, c.C, c.bank, row_window=(lo.to(dev), hi.to(dev)), exclude=True, row_logw=a2).backward(c.gout.to(dev))
    _gclose(a2.grad, c.ref("excl", c.a, (lo, hi), True)[0], "a.grad, weights only, excluded class windows")


def test_autograd_graph_tensors(ops, dev):
    """a = beta[sy] (a learned class prior), a = param + const_mask with -inf in the mask, a in fp64."""
    c = _case(ops, dev, SHAPES[1])
    g = torch.Generator().manual_seed(3)
    gout = c.gout.to(dev)
    # beta[sy]
    beta0 = torch.randn(c.C, generator=g)
    beta = beta0.to(dev).requires_grad_(True)
    ops.nw_head_bank(c.q, c.s, c.sy, c.C, c.bank, row_logw=beta[c.sy]).backward(gout)
    b64 = beta0.double().requires_grad_(True)
    out, _ = _head_f64(c.q0, c.s0, c.sy0, c.C, b64[c.sy0])
    rb, = torch.autograd.grad((out * c.gout.double()).sum(), b64)
    _gclose(beta.grad, rb, "beta.grad of a = beta[sy]")
    # param + mask
    p0 = 0.5 * torch.randn(c.N, generator=g)
    mask = torch.zeros(c.N)
    mask[c.sy0 == DEAD_CLASS] = NEG_INF
    mask[5::11] = NEG_INF
    param = p0.to(dev).requires_grad_(True)
    ops.nw_head_bank(c.q, c.s, c.sy, c.C, c.bank, row_logw=param + mask.to(dev)).backward(gout)
    rga = c.ref("param+mask", p0 + mask)[0]
    _gclose(param.grad, rga, "param.grad of a = param + mask")
    assert _positive_zero(param.grad[(mask == NEG_INF).to(dev)])
    # fp64 weights: the gradient comes back in fp64
    a64 = c.a.double().to(dev).requires_grad_(True)
    ops.nw_head_bank(c.q, c.s, c.sy, c.C, c.bank, row_logw=a64).backward(gout)
    assert a64.grad.dtype == torch.float64
    _gclose(a64.grad, c.ref("std", c.a)[0], "a.grad in fp64")


def test_write_between_forward_and_backward_is_refused(ops, dev):
    c = _case(ops, dev, SHAPES[1])
    a = c.a.to(dev).requires_grad_(True)
    out = ops.nw_head_bank(c.q, c.s, c.sy, c.C, c.bank, row_logw=a)
    with torch.no_grad():
        a[5] = 0.25
    with pytest.raises(RuntimeError, match="row_logw"):
        out.sum().backward()
    out = ops.nw_head_bank(c.q, c.s, c.sy, c.C, c.bank, row_logw=a)
    out.sum().backward()
    assert bool(torch.isfinite(a.grad).all())


def test_refused_where_the_kernel_does_not_serve(ops, dev):
    c = _case(ops, dev, SHAPES[1])
    a = c.a.to(dev).requires_grad_(True)
    half = ops.SplitBank(c.s, labels=c.sy, precision="fp16") if c.d % 64 == 0 and c.d >= 192 else None
    perm = torch.randperm(c.N, generator=torch.Generator().manual_seed(2)).to(dev)
    unsorted = ops.SplitBank(c.s, labels=c.sy[perm])
    for bank, sy in ((half, c.sy), (unsorted, c.sy[perm])):
        if bank is None:
            continue
        with pytest.raises(ops.NWHipError, match=r"nw_scores \+ a \+ nw_aggregate"):
            ops.nw_head_bank(c.q, c.s, sy, c.C, bank, row_logw=a)
    s20, sy20 = c.s[:20].contiguous(), c.sy[:20].contiguous()
    with pytest.raises(ops.NWHipError, match=r"nw_scores \+ a \+ nw_aggregate"):
        ops.nw_head_bank(c.q, s20, sy20, c.C, ops.SplitBank(s20, labels=sy20), row_logw=a[:20])


# ------------------------------------------------------------------------------------------------ 7. no B x N allocation
def test_no_score_matrix_is_allocated(ops, dev):
    B, N, d, C = 256, 65536, 64, 7
    g = torch.Generator().manual_seed(1)
    s = torch.randn(N, d, generator=g).to(dev)
    sy0 = (torch.arange(N) % C).sort().values
    sy = sy0.to(dev)
    q = torch.randn(B, d, generator=g).to(dev)
    t = torch.randint(0, C, (B,), generator=g).to(dev)
    a0 = _std_logw(sy0, dead_class=None).to(dev)
    bank = ops.SplitBank(s, labels=sy)
    matrix = B * N * 4
    # the forward's scratch is the process-wide buffer of every inference call of this shape: warmed, like the bank
    ops._WS_CACHE.clear()
    with torch.no_grad():
        ops.nw_head(q, s, sy, C, support_cache=bank, row_logw=a0)
    a = a0.clone().requires_grad_(True)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.memory_allocated(dev)
    F.nll_loss(ops.nw_head_bank(q, s, sy, C, bank, row_logw=a), t).backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(dev) - before
    print(f"MEM weights-only nw_head_bank step {peak} bytes, one score matrix {matrix} bytes")
    assert peak < matrix // 4 and bool(torch.isfinite(a.grad).all()) and float(a.grad.abs().max()) > 0


# ------------------------------------------------------------------------------------------------ 8. NWNet
class _DS(torch.utils.data.Dataset):
    def __init__(self, data, targets, C):
        self.data, self.targets, self.num_classes = data, list(targets), C

    def __len__(self):
        return len(self.targets)

    def __getitem__(self, i):
        return self.data[i], self.targets[i]


def _toy_net(dev, counts, din=48, d=64, **kw):
    from nwhead_amd.nwhead.nw import NWNet
    g = torch.Generator().manual_seed(5)
    C = len(counts)
    targets = [c for c, n in enumerate(counts) for _ in range(n)]
    perm = torch.randperm(len(targets), generator=g).tolist()
    targets = [targets[i] for i in perm]
    data = torch.randn(len(targets), din, generator=g)
    feat = nn.Linear(din, d)
    with torch.no_grad():
        feat.weight.copy_(torch.randn(d, din, generator=g) * din ** -0.5)
        feat.bias.copy_(torch.randn(d, generator=g) * 0.1)
    net = NWNet(feat, C, support_dataset=_DS(data, targets, C), n_shot=2, n_way=C, n_shot_full=max(counts), device="cuda:0", **kw).to(dev)
    net.eval()
    np.random.seed(11)
    net.precompute()
    return net, g, din


def test_nwnet_learnable_weights(ops, dev, launches):
    C, n = 6, 40
    net, g, din = _toy_net(dev, [n] * C)
    N = net.full_feat.shape[0]
    B = 24
    x = torch.randn(B, din, generator=g).to(dev)
    sy0 = net.full_y.cpu()
    w = 0.5 * torch.randn(N, generator=g)
    assert "support_logw" not in net.state_dict()
    with pytest.raises(ValueError, match="outside the parameter"):
        net.set_support_weights(torch.where(torch.arange(N) % 9 == 0, torch.tensor(NEG_INF), w), learnable=True)
    assert "support_logw" not in net.state_dict() and net.support_weights is None
    # learnable=False with the same values: the prediction learnable=True must give bit for bit
    net.set_support_weights(w)
    with torch.no_grad():
        plain = net.predict(x, 'full')
        rows = torch.randint(0, N, (B,), generator=g)
        rows[::4] = -1
        plain_loo = net.predict(x, 'full', leave_out=rows.to(dev))
    net.set_support_weights(w, learnable=True)
    assert "support_logw" in net.state_dict() and "support_logw" in dict(net.named_parameters())
    assert isinstance(net.support_logw, nn.Parameter) and net.support_logw.device.type == "cuda"
    del launches[:]
    with torch.no_grad():
        assert torch.equal(net.predict(x, 'full'), plain)
        assert torch.equal(net.predict(x, 'full', leave_out=rows.to(dev)), plain_loo)
    assert set(launches) == {FWD}
    net.zero_grad()
    net.predict(x, 'full').sum().backward()                             # read detached: nothing lands on the parameter
    assert net.support_logw.grad is None and net.featurizer.weight.grad is not None
    # forward_bank: a gradient on the parameter (and on the featurizer), against fp64
    del launches[:]
    gout = torch.randn(B, C, generator=g)
    net.zero_grad()
    net.forward_bank(x).backward(gout.to(dev))
    assert launches == [FWD, BWD_A]
    a64 = w.double().requires_grad_(True)
    with torch.no_grad():
        qfeat = net.featurizer(x).cpu()
    out, _ = _head_f64(qfeat, net.full_feat.cpu(), sy0, C, a64)
    rga, = torch.autograd.grad((out * gout.double()).sum(), a64)
    _gclose(net.support_logw.grad, rga, "support_logw.grad through forward_bank")
    assert net.featurizer.weight.grad is not None and bool(torch.isfinite(net.featurizer.weight.grad).all())
    # a frozen featurizer: the gq-free variant
    for p in net.featurizer.parameters():
        p.requires_grad_(False)
    del launches[:]
    net.zero_grad()
    net.forward_bank(x, leave_out=rows.to(dev)).backward(gout.to(dev))
    assert launches == [FWD, BWD_A + "(gq=NULL)"]
    lo = rows.clamp(min=0)
    out, _ = _head_f64(qfeat, net.full_feat.cpu(), sy0, C, a64, (lo, torch.where(rows < 0, lo, lo + 1)), True)
    rga, = torch.autograd.grad((out * gout.double()).sum(), a64)
    _gclose(net.support_logw.grad, rga, "support_logw.grad, frozen featurizer, leave_out")
    # an optimizer step moves what predict reads
    torch.optim.SGD([net.support_logw], lr=0.5).step()
    with torch.no_grad():
        assert not torch.equal(net.predict(x, 'full'), plain)
    # kept by refresh_bank, cleared by precompute()
    net.refresh_bank(rows.to(dev), feats=net.full_feat[rows.clamp(min=0).to(dev)].clone())
    assert "support_logw" in net.state_dict()
    net.precompute()
    assert "support_logw" not in net.state_dict() and net.support_weights is None


def test_nwnet_fp16_bank_refuses(ops, dev):
    net, g, din = _toy_net(dev, [40] * 4, d=192, full_precision="fp16")
    N = net.full_feat.shape[0]
    net.set_support_weights(torch.zeros(N), learnable=True)
    x = torch.randn(8, din, generator=g).to(dev)
    with pytest.raises(ops.NWHipError, match=r"nw_scores \+ a \+ nw_aggregate"):
        net.forward_bank(x)
    with torch.no_grad():                                  # inference over the fp16 bank reads them detached, as before
        assert bool(torch.isfinite(net.predict(x, 'full')).all())
