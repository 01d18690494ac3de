"""The head's backward (backward.hip, bwd_split.hip) under upstream gradients other than nll_loss's, and at
the edges of its route rules, through ops.nw_head (the C ABI) against fp64 autograd of the oracle.

Every other backward test feeds the kernels the gradient of F.nll_loss: one non-zero entry per row, all equal to -1/B.  Here
the rows of `gout` are dense, of mixed sign, of very different magnitude (per-sample weights), zero (masked samples), and laid
out the way autograd really hands them over; the shapes go past 64 KiB of dynamic LDS in the coefficient kernel, to the LDS
limit of the split route, to the class limit of the launcher, across the 256/1024-thread switch and the default thresholds.
Last, the backward over a workspace filled with NaN, at the smallest shapes that reach every area of its map.

Bar (the suite's bar for head gradients, test_fuzz_gpu.py): rtol = atol = 1e-4 on values divided by max(|ref|.max(), 1e-3);
logit_scale.grad: rtol 1e-4, atol 1e-6.  Each case runs on the route it names and ASSERTS that it does:
  valu   NW_BWD_NO_MFMA=1      plain VALU products
  mfma   NW_BWD_SPLIT=0        fp32 matrix cores (B N d >= 2^22, d % 4 == 0)
  split  default (NW_BWD_SPLIT=1 below B = 64): split-fp16 rows, per-row exponents E_b, one batch exponent G

Measured on the MI355X (largest normalised error per route over this file): valu 2.7e-5, mfma 1.8e-5, split 2.3e-5, and
7.5e-5 on every route for out.sum(), whose gq nearly cancels.  Each assertion was shown, on the host with an
fp32 restatement of the head in the device's place, to trip under the fault it is there for: only the target class of gout
used (every parity check); one E_b for the whole batch (gq / w in test_rows_of_different_magnitude, the bit-equality in
test_power_of_two_row_weights_scale_gq_exactly); no zero-row rule for ascale (gs at the 2^-10 magnitude in test_masked_rows);
dP of an absent class read into t (the bit-equality in test_dense_upstream_gradient, and nothing else).
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_fuzz_gpu import _clip_head_f64

pytestmark = pytest.mark.gpu

KINDS = ("euclidean", "hypersphere_euclidean", "cosine", "dotproduct", "clip")
ROUTES = ("valu", "mfma", "split")
LS0 = float(np.log(1 / 0.07))
# the smallest shapes of the suite with ragged tiles on every route (all have B N d >= 2^22 and d % 32 == 0)
SHAPES = [(64, 1024, 64, 5), (129, 257, 160, 1000), (33, 4099, 64, 7)]
ENV = ("NW_BWD_SPLIT", "NW_BWD_NO_MFMA")


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


@pytest.fixture(scope="module")
def L():
    from nwhead_amd import _lib
    _lib.load()
    return _lib


@pytest.fixture
def take_route(L):
    """take_route(name, B): set the switches that put the next backward on `name` ('default': none of them)."""
    saved = {k: os.environ.get(k) for k in ENV}

    def take(name, B=64):
        for k in ENV:
            os.environ.pop(k, None)
        if name == "valu":
            os.environ["NW_BWD_NO_MFMA"] = "1"
        elif name == "mfma":
            os.environ["NW_BWD_SPLIT"] = "0"
        elif name == "split" and B < 64:
            os.environ["NW_BWD_SPLIT"] = "1"
        else:
            assert name in ("split", "default")
        L.sync_knobs()
    yield take
    for k, v in saved.items():
        os.environ.pop(k, None)
        if v is not None:
            os.environ[k] = v
    L.sync_knobs()


def route_of(L, B, N, d, C, sup=0):
    """The route the NEXT backward of this shape takes under the current switches: the library's own plan."""
    L.sync_knobs()
    return L.BWD_ROUTES[L.bwd_plan(B, N, d, C, sup).route]


WORST = {}   # route -> (largest normalised error seen, where)


@pytest.fixture(scope="module", autouse=True)
def report_worst():
    """After the module: the largest normalised error per route (the figures of DESIGN.md 4.6); drops the last fp64 graph."""
    yield
    _CASE.clear()
    for route, (err, what) in sorted(WORST.items()):
        print(f"WORST {route:5s} {err:.3e} {what}")


def close(got, ref, route, what, ls=False):
    got, ref = got.detach().cpu().double().numpy(), ref.detach().double().numpy()
    assert np.isfinite(got).all(), what
    if ls:
        print(f"ERR {route:5s} {float(abs(got - ref)) / max(float(abs(ref)), 1e-30):.3e} (relative) {what}")
        np.testing.assert_allclose(got, ref, rtol=1e-4, atol=1e-6, err_msg=what)
        return
    scale = max(float(np.abs(ref).max()), 1e-3)
    err = float(np.abs(got - ref).max()) / scale
    if err > WORST.get(route, (0.0, ""))[0]:
        WORST[route] = (err, what)
    print(f"ERR {route:5s} {err:.3e} {what}")
    np.testing.assert_allclose(got / scale, ref / scale, rtol=1e-4, atol=1e-4, err_msg=what)


class Case:
    """Inputs of one (shape, kind) and the fp64 graph of the oracle head over them; reference gradients of any loss of the
    head's output come from that one graph (computed once, never modified)."""

    def __init__(self, O, B, N, d, C, kind, batched=False, seed=0):
        g = torch.Generator().manual_seed(1000 * seed + B + N + d)
        self.shape, self.kind, self.batched = (B, N, d, C), kind, batched
        q0 = torch.randn(B, d, generator=g)
        s0 = torch.randn(B, N, d, generator=g) if batched else torch.randn(N, d, generator=g)
        if kind == "dotproduct":       # keep |score| O(1..10): the softmax of raw dot products is a one-hot otherwise
            q0, s0 = q0 * d ** -0.25, s0 * d ** -0.25
        self.q0, self.s0 = q0, s0
        self.sy = torch.randint(0, C, (B, N) if batched else (N,), generator=g)
        self.q = q0.double().requires_grad_(True)
        self.s = s0.double().requires_grad_(True)
        self.ls = torch.tensor(LS0, dtype=torch.float64, requires_grad=True)
        self.out = _clip_head_f64(self.q, self.s, self.sy, C, self.ls) if kind == "clip" else \
            O.nw_head_f64(self.q, self.s, self.sy, C, kind, LS0)
        self.memo = {}

    def ref(self, tag, loss):
        """(gq, gs, gls or None) of loss(out) in fp64."""
        if tag not in self.memo:
            ins = (self.q, self.s) + ((self.ls,) if self.kind == "clip" else ())
            g = torch.autograd.grad(loss(self.out), ins, retain_graph=True)
            self.memo[tag] = tuple(g) + ((None,) if self.kind != "clip" else ())
        return self.memo[tag]

    def gpu(self, ops, dev, loss, rows=None):
        """The same loss through ops.nw_head on the device (rows: a subset of the queries)."""
        C, kind = self.shape[3], self.kind
        sel = slice(None) if rows is None else rows
        q = self.q0[sel].to(dev).requires_grad_(True)
        s = (self.s0[sel] if self.batched else self.s0).to(dev).requires_grad_(True)
        sy = (self.sy[sel] if self.batched else self.sy).to(dev)
        ls = torch.tensor(LS0, device=dev, requires_grad=True) if kind == "clip" else None
        try:
            loss(ops.nw_head(q, s, sy, C, kind, ls)).backward()
            torch.cuda.synchronize()
        except RuntimeError as e:        # a device fault ends the session: nothing more is launched on a faulted device
            if "HIP error" in str(e) or "illegal memory access" in str(e):
                pytest.exit(f"device fault in {self.shape} {kind}: {e}", returncode=3)
            raise
        return q.grad, s.grad, (ls.grad if ls is not None else None)


_CASE = {}


def case_of(O, B, N, d, C, kind, batched=False):
    """One fp64 graph alive at a time (the large ones hold (B, N, d) doubles several times over)."""
    key = (B, N, d, C, kind, batched)
    if key not in _CASE:
        _CASE.clear()
        _CASE[key] = Case(O, B, N, d, C, kind, batched)
    return _CASE[key]


def dense(B, C, seed=7):
    return torch.randn(B, C, generator=torch.Generator().manual_seed(seed))


def weighted(G):
    """loss(out) = (out * G).sum(): the upstream gradient is G, whatever out is."""
    return lambda out: (out * G.to(out)).sum()


def check(c, ops, dev, route, tag, loss, what):
    got, ref = c.gpu(ops, dev, loss), c.ref(tag, loss)
    close(got[0], ref[0], route, f"gq {what}")
    close(got[1], ref[1], route, f"gs {what}")
    if c.kind == "clip":
        close(got[2], ref[2], route, f"gls {what}", ls=True)
    return got, ref


# ------------------------------------------------------------------------------------------ 1 (a) dense upstream gradient
@pytest.mark.parametrize("route", ROUTES)                # (the first mark varies fastest: one fp64 graph serves three routes)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B,N,d,C", SHAPES)
def test_dense_upstream_gradient(dev, ops, O, L, take_route, B, N, d, C, kind, route):
    """gout = randn(B, C): the coefficient kernel's dP = gout exp(-out) over the whole row, mixed signs.  Entries of gout on
    classes that no support carries (out = log 1e-12, a factor 1e12) must change NOTHING: the same call with those entries
    zeroed gives bit-equal gradients."""
    take_route(route, B)
    assert route_of(L, B, N, d, C) == route
    c = case_of(O, B, N, d, C, kind)
    G = dense(B, C)
    what = f"dense {kind} {(B, N, d, C)}"
    got, ref = check(c, ops, dev, route, "dense", weighted(G), what)
    if kind == "euclidean" and route == "valu":          # a second, closed-form reference: no slip in this file's own graph
        gx, gs = O.nw_head_bwd_f64(c.q0, c.s0, c.sy, C, G)
        for a, b in ((gx, ref[0]), (gs, ref[1])):
            assert float((a - b).abs().max() / b.abs().max()) < 1e-9
    present = torch.bincount(c.sy, minlength=C) > 0
    assert bool(present.all()) == (C <= 7)               # C = 1000 over 257 supports: most classes are carried by nobody
    if not bool(present.all()):
        assert route_of(L, B, N, d, C) == route
        got0 = c.gpu(ops, dev, weighted(G * present))
        assert torch.equal(got[0], got0[0]) and torch.equal(got[1], got0[1]), f"absent classes leak: {what}"
        if kind == "clip":
            assert torch.equal(got[2], got0[2])


# ------------------------------------------------------------------------------------------ 1 (b) rows of different magnitude
def row_weights(B, seed=11):
    u = torch.rand(B, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    return (10.0 ** (12.0 * u - 6.0)).float()          # log-uniform over 1e-6 .. 1e6


@pytest.mark.parametrize("route", ROUTES)                # (the first mark varies fastest: one fp64 graph serves three routes)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B,N,d,C", SHAPES)
def test_rows_of_different_magnitude(dev, ops, O, L, take_route, B, N, d, C, kind, route):
    """gout = w[:, None] G with per-sample weights over twelve decades.  Row b of gq is linear in row b of gout, so
    gq / w is held to the bar of the unweighted call: under one global scale a row weighted 1e-6 could be 100 % wrong."""
    take_route(route, B)
    assert route_of(L, B, N, d, C) == route
    c = case_of(O, B, N, d, C, kind)
    w = row_weights(B)
    Gw = w[:, None] * dense(B, C)                         # (fp32, as the device sees it)
    loss = weighted(Gw)
    what = f"weighted {kind} {(B, N, d, C)}"
    got, ref = c.gpu(ops, dev, loss), c.ref("weighted", loss)
    w64 = w.double()[:, None]
    close(got[0].cpu().double() / w64, ref[0] / w64, route, f"gq/w {what}")
    close(got[1], ref[1], route, f"gs {what}")
    if kind == "clip":
        close(got[2], ref[2], route, f"gls {what}", ls=True)


# ------------------------------------------------------------------------------------------ 1 (c) power-of-two row weights
@pytest.mark.parametrize("route", ROUTES)                # (the first mark varies fastest: one fp64 graph serves three routes)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B,N,d,C", SHAPES)
def test_power_of_two_row_weights_scale_gq_exactly(dev, ops, O, L, take_route, B, N, d, C, kind, route):
    """w_b = 2^k_b, k_b in [-12, 12]: every operation on a row of the coefficient kernel and of the first product is a
    product with, or a sum of, values carrying the same power of two (E_b moves by exactly k_b and ascale[b] undoes it), so
    gq[b] is BIT-equal to 2^k_b times the unweighted gq[b].  Fails if one row's scale ever leaks into another's.  gs goes
    through the batch exponent G and is held to the bar."""
    take_route(route, B)
    assert route_of(L, B, N, d, C) == route
    c = case_of(O, B, N, d, C, kind)
    G = dense(B, C)
    k = torch.randint(-12, 13, (B,), generator=torch.Generator().manual_seed(13))
    w = torch.ldexp(torch.ones(B), k)
    loss = weighted(w[:, None] * G)                       # exact products
    plain = c.gpu(ops, dev, weighted(G))
    got, ref = c.gpu(ops, dev, loss), c.ref("pow2", loss)
    what = f"pow2 {kind} {(B, N, d, C)}"
    want = torch.ldexp(plain[0].cpu(), k[:, None].expand(B, d))
    bad = (got[0].cpu() != want).any(dim=1)
    assert not bool(bad.any()), f"{what} [{route}]: rows {bad.nonzero().flatten().tolist()[:8]} of gq are not 2^k times the unweighted"
    close(got[1], ref[1], route, f"gs {what}")
    if kind == "clip":
        close(got[2], ref[2], route, f"gls {what}", ls=True)


# ------------------------------------------------------------------------------------------ 1 (d) masked rows
def row_mask(B):
    """A third of the rows: the first, the last, a whole 32-row block where the batch has one to spare, the rest at random."""
    m = torch.zeros(B, dtype=torch.bool)
    m[0] = m[-1] = True
    if B >= 96:
        m[32:64] = True
    order = torch.randperm(B, generator=torch.Generator().manual_seed(17))
    for b in order.tolist():
        if int(m.sum()) >= (B + 2) // 3:
            break
        m[b] = True
    return m


@pytest.mark.parametrize("route", ROUTES)                # (the first mark varies fastest: one fp64 graph serves three routes)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B,N,d,C", SHAPES)
def test_masked_rows(dev, ops, O, L, take_route, B, N, d, C, kind, route):
    """Zero rows of gout (masked samples): those rows of gq are exactly 0, everything is finite, gs meets the bar -- and
    equals, at the bar, the gs of the call made with the unmasked queries only (a zero row must not take part in the batch
    exponent G: DESIGN.md 4.6, the zero-row rule of ascale)."""
    take_route(route, B)
    assert route_of(L, B, N, d, C) == route
    c = case_of(O, B, N, d, C, kind)
    m = row_mask(B)
    assert m[0] and m[-1] and B // 3 <= int(m.sum()) <= B // 2 and (B < 96 or bool(m[32:64].all()))
    keep = (~m).nonzero().flatten()
    # at the magnitude of a sum-reduced loss and at that of a mean-reduced one (2^-10): the smaller the coefficients, the
    # further a zero row's 2^0 would sit from the other rows' 2^-E_b -- at 2^-10 the split images of every other query
    # underflow without the zero-row rule (gs wrong by 2e-4 to 6e-4 of its scale at these shapes, worked out on the host)
    for tag, scale in (("masked", 1.0), ("masked-small", 2.0 ** -10)):
        Gm = dense(B, C) * (~m)[:, None] * scale
        what = f"{tag} {kind} {(B, N, d, C)}"
        got, ref = check(c, ops, dev, route, tag, weighted(Gm), what)
        assert bool((got[0].cpu()[m] == 0).all()), f"{what}: a masked row of gq is not exactly zero"
        sub = c.gpu(ops, dev, weighted(Gm[keep]), rows=keep)          # (whatever route the smaller batch takes)
        close(sub[0], ref[0][keep], route, f"gq of the unmasked-only call {what}")
        close(got[1], sub[1].cpu().double(), route, f"gs against the unmasked-only call {what}")


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("kind", ("euclidean", "clip"))
def test_all_rows_masked_gives_exact_zeros(dev, ops, O, L, take_route, kind, route):
    B, N, d, C = SHAPES[0]
    take_route(route, B)
    assert route_of(L, B, N, d, C) == route
    c = case_of(O, B, N, d, C, kind)
    got = c.gpu(ops, dev, weighted(torch.zeros(B, C)))
    for g in got[:2] + ((got[2],) if kind == "clip" else ()):
        assert bool((g == 0).all()) and bool(torch.isfinite(g).all())


# ------------------------------------------------------------------------------------------ 1 (e) layouts autograd produces
def _loss_sum(out):
    return out.sum()                                       # an expanded, stride-0 gradient


def _loss_transposed(out):
    Gt = torch.randn(out.shape[1], out.shape[0], generator=torch.Generator().manual_seed(19))
    return (out.t() * Gt.to(out)).sum()                    # a transposed one


def _loss_twice(out):
    G = dense(*out.shape, seed=23).to(out)
    return (out * G).sum() + 0.1 * (out * out).sum()       # two uses of out: accumulated gradients


def _loss_smoothed(out):
    t = torch.randint(0, out.shape[1], (out.shape[0],), generator=torch.Generator().manual_seed(29)).to(out.device)
    return F.cross_entropy(out, t, label_smoothing=0.1)    # the realistic dense case


@pytest.mark.parametrize("loss,kind,route", [(_loss_sum, "euclidean", "split"), (_loss_sum, "euclidean", "mfma"),
                                             (_loss_sum, "euclidean", "valu"), (_loss_transposed, "cosine", "mfma"),
                                             (_loss_twice, "hypersphere_euclidean", "valu"), (_loss_smoothed, "clip", "split"),
                                             (_loss_smoothed, "dotproduct", "mfma")])
def test_gradient_layouts_of_autograd(dev, ops, O, L, take_route, loss, kind, route):
    B, N, d, C = SHAPES[0]
    take_route(route, B)
    assert route_of(L, B, N, d, C) == route
    check(case_of(O, B, N, d, C, kind), ops, dev, route, loss.__name__, loss, f"{loss.__name__} {kind}")


# ------------------------------------------------------------------------------------------ 1 (f) per-query supports
@pytest.mark.parametrize("B,N,d,C", [(3, 3000, 36, 7), (5, 2049, 16, 3)])
@pytest.mark.parametrize("kind", ("euclidean", "cosine", "clip"))
def test_per_query_supports_dense_gradient(dev, ops, O, L, take_route, B, N, d, C, kind):
    """(B, N, d) supports with (B, N) labels: nw_bwd_gs_batched_kernel past N = 700, 1024-thread coefficient kernel."""
    take_route("default")
    assert route_of(L, B, N, d, C, sup=1) == "valu" and N >= 2048
    check(case_of(O, B, N, d, C, kind, batched=True), ops, dev, "valu", "dense", weighted(dense(B, C)),
          f"per-query {kind} {(B, N, d, C)}")


# ------------------------------------------------------------------------------------------ 2  edges of the route rules
def nll(B, C, sy=None, seed=31):
    """nll_loss on random targets; with far more classes than supports the targets are drawn from the supports' labels (a
    target that no support carries has an exactly zero gradient: B such rows would compare nothing)."""
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(0, C, (B,), generator=g) if sy is None else sy.flatten()[torch.randint(0, sy.numel(), (B,), generator=g)]
    return lambda out: F.nll_loss(out, t.to(out.device))


def alternate(i, B, C, sy=None):
    """nll and a dense gradient in turn, so that both keep being exercised."""
    return ("nll", nll(B, C, sy)) if i % 2 == 0 else ("dense", weighted(dense(B, C)))


def coeff_lds_bytes(N, C, route):
    return 4 * (80 + C + ((N + 31) // 32 * 32 if route == "split" else 0))


@pytest.mark.parametrize("i,kind", list(enumerate(KINDS)))
def test_coefficient_kernel_above_64k_of_lds_on_the_split_route(dev, ops, O, L, take_route, i, kind):
    """B = 16, N = 20000, d = 32, C = 5: 80 340 bytes of dynamic LDS, default route, no switch; every kind is its own kernel
    instantiation.  Also the first product's 16-way K split over a long K."""
    B, N, d, C = 16, 20000, 32, 5
    take_route("default")
    assert route_of(L, B, N, d, C) == "split" and coeff_lds_bytes(N, C, "split") == 80340 > 64 * 1024
    tag, loss = alternate(i, B, C)
    check(case_of(O, B, N, d, C, kind), ops, dev, "split", tag, loss, f"lds80k {tag} {kind}")


@pytest.mark.parametrize("i,N,route", [(0, 38300, "split"), (1, 38305, "mfma")])
@pytest.mark.parametrize("kind", ("euclidean", "cosine"))
def test_lds_limit_of_the_split_route(dev, ops, O, L, take_route, i, N, route, kind):
    """C = 16, d = 32, B = 16.  N = 38300: ld = 38304, 80 + ld + C floats = exactly 150 KiB, the last row that splits;
    N = 38305: ld = 38336, the fp32 matrix cores.  No switch: the rule decides."""
    B, d, C = 16, 32, 16
    take_route("default")
    assert route_of(L, B, N, d, C) == route
    assert (coeff_lds_bytes(N, C, "split") <= 150 * 1024) == (route == "split")
    if route == "split":
        assert coeff_lds_bytes(N, C, "split") == 150 * 1024
    tag, loss = alternate(i + (kind == "cosine"), B, C)
    try:
        check(case_of(O, B, N, d, C, kind), ops, dev, route, tag, loss, f"ldslimit N={N} {tag} {kind}")
    finally:
        _CASE.clear()                                        # ~20 M differences in fp64: gone before the next case


@pytest.mark.parametrize("i,B,N,d,C,switch,route,kind", [
    (0, 8, 300, 16, 20000, "default", "valu", "euclidean"),          # 80 320 bytes
    (1, 8, 300, 16, 20000, "default", "valu", "dotproduct"),
    # 80 + 1024 + 30000 floats = 124 416 bytes is UNDER the split route's 150 KiB: by default this shape splits ...
    (0, 64, 1000, 512, 30000, "default", "split", "euclidean"),
    (1, 64, 1000, 512, 30000, "default", "split", "dotproduct"),
    # ... and runs the fp32 matrix cores (120 320 bytes) with the split route switched off
    (1, 64, 1000, 512, 30000, "mfma", "mfma", "euclidean"),
    (0, 64, 1000, 512, 30000, "mfma", "mfma", "dotproduct"),
    # 80 + 1024 + 37500 floats > 150 KiB: the LDS rule alone keeps it off the split route (150 320 bytes, fp32 matrix cores)
    (0, 64, 1000, 512, 37500, "default", "mfma", "euclidean"),
])
def test_many_classes(dev, ops, O, L, take_route, i, B, N, d, C, switch, route, kind):
    """dP of 20 000 to 37 500 classes in LDS (80 to 150 KB), most of them carried by no support."""
    take_route(switch, B)
    assert route_of(L, B, N, d, C) == route
    if C == 37500:
        assert 4 * (80 + 1024 + C) > 150 * 1024 and N >= 256 and B >= 16 and d % 32 == 0      # the LDS rule alone keeps it off
    assert coeff_lds_bytes(N, C, route) > 64 * 1024
    c = case_of(O, B, N, d, C, kind)
    tag, loss = alternate(i, B, C, c.sy)
    try:
        check(c, ops, dev, route, tag, loss, f"classes C={C} {tag} {kind} [{switch}]")
    finally:
        _CASE.clear()


def test_class_limit_of_the_launcher(dev, ops, O, L, take_route):
    """(80 + C) floats <= 160 KiB: C = 40880 is the last class count the backward takes, 40881 is refused with
    NW_ERR_UNSUPPORTED and no gradient is written.  A guard: the kernel is not extended."""
    from nwhead_amd._lib import NWHipError
    B, N, d = 2, 30, 8
    take_route("default")
    assert route_of(L, B, N, d, 40880) == "valu" and 4 * (80 + 40880) == 160 * 1024
    check(case_of(O, B, N, d, 40880, "euclidean"), ops, dev, "valu", "dense", weighted(dense(B, 40880)), "C=40880")
    _CASE.clear()
    C = 40881
    g = torch.Generator().manual_seed(3)
    q = torch.randn(B, d, generator=g).to(dev).requires_grad_(True)
    s = torch.randn(N, d, generator=g).to(dev).requires_grad_(True)
    out = ops.nw_head(q, s, torch.randint(0, C, (N,), generator=g).to(dev), C, "euclidean")
    assert bool(torch.isfinite(out).all())
    with pytest.raises(NWHipError, match=r"unsupported score kind or size \(status -2\)"):
        out.backward(dense(B, C).to(dev))
    assert q.grad is None and s.grad is None


def test_aggregate_backward_with_many_classes(dev):
    """nw_aggregate_bwd_f32 has a launch site of its own: a callable kernel module at C = 20000, N = 3000 (80 320 bytes,
    1024 threads)."""
    import torch.nn as nn
    from nwhead_amd.nwhead.nw import NWHead

    class L1(nn.Module):
        def forward(self, x, y):
            return -torch.cdist(x, y, p=1.0)
    B, N, d, C = 4, 3000, 8, 20000
    g = torch.Generator().manual_seed(5)
    x0, s0 = torch.randn(B, d, generator=g), torch.randn(N, d, generator=g)
    sy = torch.randint(0, C, (N,), generator=g)
    G = dense(B, C)
    x64, s64 = x0.double().requires_grad_(True), s0.double().requires_grad_(True)
    w = (-torch.cdist(x64, s64, p=1.0)).softmax(-1)
    p = torch.zeros(B, C, dtype=torch.float64).index_add(1, sy, w)                 # (= w @ one_hot(sy), without the N x C matrix)
    ref = torch.log(p + 1e-12)
    (ref * G.double()).sum().backward()
    x, s = x0.to(dev).requires_grad_(True), s0.to(dev).requires_grad_(True)
    out = NWHead(L1(), C)(x, s, sy.to(dev))
    np.testing.assert_allclose(out.detach().cpu().numpy(), ref.detach().numpy(), rtol=1e-5, atol=3e-5)
    (out * G.to(dev)).sum().backward()
    close(x.grad, x64.grad, "valu", "gx aggregate C=20000")
    close(s.grad, s64.grad, "valu", "gs aggregate C=20000")


@pytest.mark.parametrize("i,N", list(enumerate((2047, 2048, 2049, 4097))))
def test_thread_count_switch_of_the_coefficient_kernel(dev, ops, O, L, take_route, i, N):
    """256 threads below N = 2048, 1024 from there, on the VALU route: the four-wide unrolled, clamped tail one element
    before, at and after the switch, and at 4 * 1024 + 1, one element into a new unrolled round."""
    B, d, C = 4, 16, 3
    take_route("default")
    assert route_of(L, B, N, d, C) == "valu"
    tag, loss = alternate(i, B, C)
    check(case_of(O, B, N, d, C, KINDS[i % 3]), ops, dev, "valu", tag, loss, f"threads N={N} {tag}")


@pytest.mark.parametrize("i,B,N,d,route", [(0, 16, 256, 1024, "split"),    # B N d = 2^22 exactly
                                           (1, 15, 280, 1024, "mfma"),     # B < 16
                                           (2, 16, 255, 1056, "mfma"),     # N < 256
                                           (3, 16, 256, 992, "valu")])     # B N d < 2^22
def test_default_thresholds(dev, ops, O, L, take_route, i, B, N, d, route):
    C = 5
    take_route("default")
    assert route_of(L, B, N, d, C) == route
    assert (B * N * d >= 2 ** 22) == (route != "valu")
    tag, loss = alternate(i, B, C)
    check(case_of(O, B, N, d, C, ("euclidean", "cosine")[i % 2]), ops, dev, route, tag, loss, f"threshold {(B, N, d)} {tag}")


# ------------------------------------------------------------------------------------------ 3  a poisoned workspace
# the smallest shapes that reach every area of the backward's workspace, with what each is there for
POISON_SHAPES = [
    (64, 1024, 64, 5),     # d % 64 == 0: the caller's bank is read; gq K-split, its reduction deferred into the gs launch
    (64, 1024, 96, 5),     # d % 32 == 0 but d % 64 != 0: the split rows are the workspace copy
    (256, 512, 64, 5),     # both products K-split: part and part2 live at once (split), one shared area (fp32 matrix cores)
]


@pytest.mark.parametrize("route", ROUTES)                # (the first mark varies fastest: one fp64 graph serves three routes)
@pytest.mark.parametrize("kind", ("euclidean", "clip"))
@pytest.mark.parametrize("B,N,d,C", POISON_SHAPES)
def test_backward_on_a_poisoned_workspace(dev, ops, O, L, take_route, B, N, d, C, kind, route):
    """The backward never clears its workspace and ops keeps one buffer per stream: whatever a kernel reads there without
    having written it is the previous call's.  Forward, then the cached buffer filled with 0xFF (NaN as a float), then
    backward(): every gradient finite, bit-equal to the same step over a zero-filled buffer, and at the bar of the oracle."""
    from ws_poison import poison_cached_workspaces
    take_route(route, B)
    plan = L.bwd_plan(B, N, d, C)
    assert route_of(L, B, N, d, C) == route and plan.total == L.load().nw_bwd_workspace_bytes(B, N, d, C, 0, 0)
    cq, cs = plan.gq_chunks, plan.gs_chunks
    if route == "valu":
        assert cq == 0 and cs == 0
    elif (B, N, d) == (64, 1024, 64):
        assert cq > 1
    elif (B, N, d) == (256, 512, 64):
        assert cq > 1 and cs > 1
        size = dict(zip(L.BWD_AREAS, zip(plan.off, plan.bytes)))
        assert (size["part"] == size["part2"]) == (route == "mfma") == bool(plan.parts_shared)
    if route == "split":
        assert plan.bytes[L.BWD_AREAS.index("s_split")] >= 4 * N * d     # reserved whether or not the bank is read
    c = case_of(O, B, N, d, C, kind)
    loss = weighted(dense(B, C))

    def zero_fill():
        ops._workspace(plan.total, dev)
        return sum(int(ws.zero_().numel()) for ws in ops._WS_CACHE.values())

    def step(fill):
        q, s = c.q0.to(dev).requires_grad_(True), c.s0.to(dev).requires_grad_(True)
        ls = torch.tensor(LS0, device=dev, requires_grad=True) if kind == "clip" else None
        out = ops.nw_head(q, s, c.sy.to(dev), C, kind, ls)
        assert fill() >= plan.total > 0
        try:
            loss(out).backward()
            torch.cuda.synchronize()
        except RuntimeError as e:        # a device fault ends the session, as in Case.gpu
            if "HIP error" in str(e) or "illegal memory access" in str(e):
                pytest.exit(f"device fault in {(B, N, d, C)} {kind}: {e}", returncode=3)
            raise
        return (q.grad, s.grad) + ((ls.grad,) if ls is not None else ())

    got, clean = step(lambda: poison_cached_workspaces(min_bytes=plan.total, device=dev)), step(zero_fill)
    what = f"poisoned {kind} {(B, N, d, C)}"
    for g, z, name in zip(got, clean, ("gq", "gs", "gls")):
        assert bool(torch.isfinite(g).all()), f"{name} {what} [{route}]"
        assert torch.equal(g, z), f"{name} {what} [{route}]: differs from the step over a zero-filled workspace"
    ref = c.ref("dense", loss)
    close(got[0], ref[0], route, f"gq {what}")
    close(got[1], ref[1], route, f"gs {what}")
    if kind == "clip":
        close(got[2], ref[2], route, f"gls {what}", ls=True)
