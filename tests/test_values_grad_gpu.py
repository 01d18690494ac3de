"""The value head at training time: ops.nw_head_values_bank -> the inference launches forward, nw_bwd_values_query_f32
(bwd_values.hip) backward, and NWNet.forward_values.

Reference: fp64 torch autograd on the CPU over oracle.nw_oracle.scores_f64 (32 queries at a time), softmax(score + a over
the admitted rows) @ values with the rows masked before the softmax and dead queries set to 0; clip carries its logit scale
in the graph.  Inputs are random normal q, s and values and a random normal upstream gradient.

Bar (the suite's bar for head gradients, test_bwd_query_gpu.py): rtol = atol = 1e-4 on values divided by
max(|ref|.max(), 1e-3); logit_scale.grad: rtol 1e-4, atol 1e-6.  Every comparison prints its normalised error and the module
prints the worst one at the end.  Every fused call runs on a workspace filled with 0xFF beforehand."""
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
# (B, N, d, T), test_head_values_gpu.py's: a partial query tile, a ragged last support tile, T padded from 5; three query
# tiles, a slab of fewer than NCH blocks, T padded to 64; the smallest bank, one stage in each product; nine stages in the T
# product
SHAPES = [(37, 1000, 64, 5), (130, 4100, 96, 40), (64, 26, 32, 1), (70, 2048, 64, 288)]
SMALL = SHAPES[0]
PATTERN = (0.0, math.log(2.0), -3.5, NEG_INF, 0.0, 1.25, -0.5)      # the standard weights of test_head_weighted_gpu.py
DEAD_CLASS = 3
C16 = 16
TILE_ROWS = 64
VALUES, SCORES, WINDOW, WEIGHTED, PLAIN = "nw_fwd_values_f32", "nw_scores_f32", "nw_fwd_window_f32", "nw_fwd_weighted_f32", "nw_fwd_f32"
BWDV, BWDQ = "nw_bwd_values_query_f32", "nw_bwd_query_f32"
SPIED = (VALUES, SCORES, WINDOW, WEIGHTED, PLAIN, BWDV, BWDQ, "nw_aggregate_f32", "nw_bank_update_rows_f32")
WORST = [0.0, ""]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "run with -m gpu on the MI355X box"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from nwhead_amd import ops as o
    assert hasattr(o, "nw_head_values_bank"), "the value head's training-time entry is missing"
    return o


@pytest.fixture(scope="module", autouse=True)
def report_worst():
    yield
    _CASES.clear()
    print(f"WORST bwd_values {WORST[0]:.3e} {WORST[1]}")


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


def close(got, ref, what, ls=False):
    got, ref = got.detach().cpu().double().numpy(), ref.detach().double().numpy()
    assert np.isfinite(got).all(), what
    if ls:
        print(f"ERR {float(abs(got - ref)) / max(float(abs(ref)), 1e-30):.3e} (relative) {what}")
        np.testing.assert_allclose(got, ref, rtol=1e-4, atol=1e-6, err_msg=what)
        return
    scale = max(float(np.abs(ref).max()), 1e-3)
    err = float(np.abs(got - ref).max()) / scale
    if err > WORST[0]:
        WORST[:] = [err, what]
    print(f"ERR {err:.3e} {what}")
    np.testing.assert_allclose(got / scale, ref / scale, rtol=1e-4, atol=1e-4, err_msg=what)


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
    """fp64 softmax(score + a over the admitted rows) @ v, differentiable in `sc`; a dead query is 0."""
    x = sc if a is None else sc + a.double()
    if keep is not None:
        x = x.masked_fill(~keep, NEG_INF)
    live = torch.isfinite(x).any(dim=1, keepdim=True)
    zero = torch.zeros_like(x)
    return torch.where(live, torch.softmax(torch.where(live, x, zero), dim=1), zero) @ v.double()


def f64_grads(q, s, v, kind, specs):
    """{name: (gq, gls or None)} in fp64 for specs = {name: dict(a=, keep=, loss=f(out, rows) -> scalar)}: 32 queries at a
    time (they are independent), the score graph of a block built once and walked once per spec."""
    from oracle import nw_oracle
    B, clip = q.shape[0], kind == "clip"
    res = {name: [torch.zeros(q.shape, dtype=torch.float64), torch.zeros((), dtype=torch.float64) if clip else None] for name in specs}
    for i in range(0, B, 32):
        rows = slice(i, min(i + 32, B))
        qb = q[rows].double().requires_grad_(True)
        ls = torch.tensor(LS0, dtype=torch.float64, requires_grad=True) if clip else None
        sc = nw_oracle.scores_f64(qb, s, "cosine" if clip else kind)
        if clip:
            sc = ls.exp() * sc
        for name, sp in specs.items():
            keep = sp.get("keep")
            out = weighted_mean_f64(sc, v, sp.get("a"), None if keep is None else keep[rows])
            gr = torch.autograd.grad(sp["loss"](out, rows), (qb,) + ((ls,) if clip else ()), retain_graph=True)
            res[name][0][rows] = gr[0]
            if clip:
                res[name][1] += gr[1]
    return {name: tuple(r) for name, r in res.items()}


def dot_loss(gout):
    """A general upstream gradient: the loss sum(out * gout)."""
    return lambda out, rows: (out * gout[rows].double()).sum()


class Case:
    """Inputs of one (shape, kind) on the CPU, the bank and the prepared values on the device, the five variants of the
    parity test (plain, weights with -inf rows, kept class window, excluded single-row window, window + weights) and their
    fp64 reference gradients (computed once)."""

    def __init__(self, ops, dev, B, N, d, T, kind):
        g = torch.Generator().manual_seed(B * 7919 + N * 31 + d + 13 * T)
        self.shape, self.kind, self.dev = (B, N, d, T), kind, dev
        self.q, self.s, self.v = torch.randn(B, d, generator=g), torch.randn(N, d, generator=g), torch.randn(N, T, generator=g)
        self.gout = torch.randn(B, T, generator=g)
        self.sy = _sorted_labels(N)
        self.a = _std_logw(self.sy)
        qy = torch.randint(0, C16, (B,), generator=g)
        qy[1] = DEAD_CLASS                           # at least one query whose class window holds switched-off rows alone
        self.lo, self.hi = torch.searchsorted(self.sy, qy), torch.searchsorted(self.sy, qy, right=True)
        self.row = (torch.arange(B) * 27 + 5) % N
        self.qd, self.sd, self.vd = self.q.to(dev), self.s.to(dev), self.v.to(dev)
        self.bank = ops.SplitBank(self.sd, labels=self.sy.to(dev))
        self.vals = ops.BankValues(self.vd, self.bank)
        self.ad = self.a.to(dev)
        cls, one = (self.lo.to(dev), self.hi.to(dev)), (self.row.to(dev), self.row.to(dev) + 1)
        # name -> (keyword arguments of the call, the reference's weights and admitted rows)
        self.variants = {
            "plain": ({}, {}),
            "weights": (dict(row_logw=self.ad), dict(a=self.a)),
            "kept class window": (dict(row_window=cls), dict(keep=_admitted(N, self.lo, self.hi, False))),
            "excluded single-row window": (dict(row_window=one, exclude=True), dict(keep=_admitted(N, self.row, self.row + 1, True))),
            "window and weights": (dict(row_window=cls, row_logw=self.ad), dict(a=self.a, keep=_admitted(N, self.lo, self.hi, False))),
        }
        self.memo = None

    def ls(self, grad=True):
        return torch.tensor(LS0, device=self.dev, requires_grad=grad) if self.kind == "clip" else None

    def parity_refs(self):
        if self.memo is None:
            self.memo = f64_grads(self.q, self.s, self.v, self.kind,
                                  {name: dict(loss=dot_loss(self.gout), **rkw) for name, (_, rkw) in self.variants.items()})
        return self.memo

    def ref(self, loss, v=None, **rkw):
        return f64_grads(self.q, self.s, self.v if v is None else v, self.kind, {"x": dict(loss=loss, **rkw)})["x"]


_CASES = {}


def case(ops, dev, shape, kind):
    if (shape, kind) not in _CASES:
        _CASES[(shape, kind)] = Case(ops, dev, *shape, kind)
    return _CASES[(shape, kind)]


def _poison(dev, B, N, d, Tp):
    from nwhead_amd import _lib
    lib = _lib.load()
    need = max(ws_poison.fwd_workspace_bytes(B, N, d, 1), int(lib.nw_fwd_values_workspace_bytes(B, N, d, Tp, 0)),
               int(lib.nw_bwd_values_query_workspace_bytes(B, N, d, Tp, 0)))
    assert need > 0 and ws_poison.poison_cached_workspaces(need, dev) >= need


def run(ops, c, gout=None, loss=None, vals=None, log=False, **kw):
    """(out, q.grad, logit_scale.grad) of ops.nw_head_values_bank under the upstream gradient `gout` (or the scalar
    loss(out)), on a poisoned workspace."""
    B, N, d, T = c.shape
    _poison(c.dev, B, N, d, T + (-T) % 32)
    q, ls = c.qd.clone().requires_grad_(True), c.ls()
    out = ops.nw_head_values_bank(q, c.sd, c.bank, c.vals if vals is None else vals, c.kind, ls, log=log, **kw)
    _poison(c.dev, B, N, d, T + (-T) % 32)
    if loss is None:
        out.backward(gout.to(c.dev))
    else:
        loss(out).backward()
    return out.detach(), q.grad, None if ls is None else ls.grad


# ------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", KINDS)
def test_parity_with_fp64(ops, dev, launches, kind, shape):
    c = case(ops, dev, shape, kind)
    refs = c.parity_refs()
    for name, (kw, _) in c.variants.items():
        n0 = len(launches)
        out, gq, gls = run(ops, c, c.gout, **kw)
        assert launches[n0:] == [WEIGHTED if "row_logw" in kw else WINDOW, VALUES, BWDV], (name, launches[n0:])
        with torch.no_grad():
            assert torch.equal(out, ops.nw_head_values(c.qd, c.sd, c.bank, c.vals, c.kind, c.ls(False), **kw)), name
        rq, rls = refs[name]
        close(gq, rq, f"gq {kind} {shape} {name}")
        if kind == "clip":
            close(gls, rls, f"gls {kind} {shape} {name}", ls=True)
    dead = ~(torch.isfinite(c.a)[None, :] & c.variants["window and weights"][1]["keep"]).any(1)
    assert dead[1] and not dead.all()            # the queries of the class that is switched off: a zero row, checked above


# ------------------------------------------------------------------------------------------------ 2. forward bits, launches, memory
def test_forward_is_the_inference_call_and_nothing_of_size_BxN_is_held(ops, dev, launches):
    shape = (130, 4100, 96, 40)
    c = case(ops, dev, shape, "euclidean")
    B, N, d, T = shape
    kw = c.variants["window and weights"][0]
    run(ops, c, c.gout, **kw)                                        # (the workspaces are cached from here on)
    with torch.no_grad():
        want = ops.nw_head_values(c.qd, c.sd, c.bank, c.vals, **kw)
        want_log = ops.nw_head_values(c.qd, c.sd, c.bank, c.vals, log=True, **kw)
    q = c.qd.clone().requires_grad_(True)
    gout = c.gout.to(dev)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    del launches[:]
    out = ops.nw_head_values_bank(q, c.sd, c.bank, c.vals, **kw)
    assert launches == [WEIGHTED, VALUES]
    out.backward(gout)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(dev) - base
    assert launches == [WEIGHTED, VALUES, BWDV] and SCORES not in launches and PLAIN not in launches
    print(f"peak allocation of one step at {shape}: {peak} bytes against B N 4 = {B * N * 4}")
    assert peak < B * N * 4
    assert torch.equal(out.detach(), want) and out.shape == (B, T) and q.grad.shape == (B, d)
    # log=True: the same node, log(out + 1e-12) behind it
    q2 = c.qd.clone().requires_grad_(True)
    logged = ops.nw_head_values_bank(q2, c.sd, c.bank, c.vals, log=True, **kw)
    assert torch.allclose(logged.detach(), want_log, rtol=0, atol=0, equal_nan=True)      # (log of a negative estimate: NaN in both)
    # nothing requires grad, or grad mode is off: nw_head_values itself
    del launches[:]
    assert torch.equal(ops.nw_head_values_bank(c.qd, c.sd, c.bank, c.vals, **kw), want)
    with torch.no_grad():
        assert torch.equal(ops.nw_head_values_bank(q, c.sd, c.bank, c.vals, **kw), want)
    assert launches == [WEIGHTED, VALUES] * 2


# ------------------------------------------------------------------------------------------------ 3. repeatability, chunks
def test_two_backward_calls_are_bit_equal(ops, dev):
    c = case(ops, dev, (130, 4100, 96, 40), "clip")
    kw = c.variants["window and weights"][0]
    _, g1, l1 = run(ops, c, c.gout, **kw)
    _, g2, l2 = run(ops, c, c.gout, **kw)
    assert torch.equal(g1, g2) and torch.equal(l1, l2)


@pytest.mark.parametrize("row_chunks", [1, 2, 3, 16])
def test_forced_chunks_meet_the_bar_and_repeat_bit_for_bit(ops, dev, row_chunks):
    from nwhead_amd import _lib
    lib = _lib.load()
    c = case(ops, dev, SMALL, "clip")
    B, N, d, T = SMALL
    assert (N + TILE_ROWS - 1) // TILE_ROWS == 16                     # 16: one chunk per support tile
    Tp = c.vals.width
    lod, hid = c.row.to(dev).int(), (c.row + 1).to(dev).int()
    ls = c.ls(False)
    with torch.no_grad():
        out, lse = ops.nw_head_values(c.qd, c.sd, c.bank, c.vals, "clip", ls, row_window=(lod, hid), exclude=True, row_logw=c.ad,
                                      return_lse=True)
    outp = F.pad(out, (0, Tp - T)).contiguous()
    goutp = F.pad(c.gout.to(dev), (0, Tp - T)).contiguous()
    need = int(lib.nw_bwd_values_query_workspace_bytes(B, N, d, Tp, row_chunks))
    assert need > 0
    st = torch.cuda.current_stream(dev).cuda_stream
    res = []
    for _ in range(2):
        ws = ws_poison.poisoned_workspace(need, dev)
        gq = torch.full((B, d), float("nan"), device=dev)
        gls = torch.full((), float("nan"), device=dev)
        rc = lib.nw_bwd_values_query_f32(c.qd.data_ptr(), c.bank.split.data_ptr(), c.bank.scale.data_ptr(), c.bank.norm2.data_ptr(),
                                         c.vals.split.data_ptr(), c.vals.scale.data_ptr(), c.ad.data_ptr(), lod.data_ptr(),
                                         hid.data_ptr(), 1, lse.data_ptr(), outp.data_ptr(), goutp.data_ptr(), gq.data_ptr(),
                                         gls.data_ptr(), ws.data_ptr(), need, B, N, d, Tp, 4, ls.data_ptr(), row_chunks, st)
        assert rc == 0
        torch.cuda.synchronize()
        res.append((gq, gls))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    rq, rls = c.ref(dot_loss(c.gout), a=c.a, keep=_admitted(N, c.row, c.row + 1, True))
    close(res[0][0], rq, f"gq row_chunks={row_chunks}")
    close(res[0][1], rls, f"gls row_chunks={row_chunks}", ls=True)


# ------------------------------------------------------------------------------------------------ 4. exact scaling
@pytest.mark.parametrize("kind", ["euclidean", "clip"])
def test_scaling_gout_by_a_power_of_two_scales_gq_exactly(ops, dev, kind):
    c = case(ops, dev, (130, 4100, 96, 40), kind)
    B = c.shape[0]
    kw = c.variants["weights"][0]
    _, gq, gls = run(ops, c, c.gout, **kw)
    assert float(gq.abs().max()) > 0
    for k in (20, -20):
        _, g2, l2 = run(ops, c, c.gout * 2.0 ** k, **kw)
        assert torch.equal(g2, gq * 2.0 ** k), f"whole, k = {k}"
        if kind == "clip":
            assert torch.equal(l2, gls * 2.0 ** k)
    per_row = 2.0 ** torch.tensor([20.0, -20.0, 0.0, 7.0, -13.0])[torch.arange(B) % 5]
    _, g3, _ = run(ops, c, c.gout * per_row[:, None], **kw)
    assert torch.equal(g3, gq * per_row.to(dev)[:, None]), "per row"


# ------------------------------------------------------------------------------------------------ 5. exact zeros
@pytest.mark.parametrize("kind", KINDS)
def test_dead_queries_and_zero_gradients_give_exact_zeros(ops, dev, kind):
    c = case(ops, dev, SMALL, kind)
    B, N, d, T = SMALL
    # every third query: an empty kept window; the queries of the switched-off class: every admitted row at -inf
    lo, hi = c.lo.clone(), c.hi.clone()
    empty = torch.arange(B) % 3 == 0
    hi[empty] = lo[empty]
    keep = _admitted(N, lo, hi, False)
    dead = ~(keep & torch.isfinite(c.a)[None, :]).any(1)
    assert empty.any() and (dead & ~empty).any() and not dead.all()
    kw = dict(row_window=(lo.to(dev), hi.to(dev)), row_logw=c.ad)
    out, gq, gls = run(ops, c, c.gout, **kw)
    assert bool(torch.isfinite(gq).all()) and bool((out.cpu()[dead] == 0).all())
    assert bool((gq.cpu()[dead] == 0).all()) and bool((gq.cpu()[~dead].abs().amax(1) > 0).all())
    rq, rls = c.ref(dot_loss(c.gout), a=c.a, keep=keep)
    close(gq, rq, f"gq {kind} dead queries")
    if kind == "clip":
        close(gls, rls, f"gls {kind} dead queries", ls=True)
    # an all-zero upstream gradient, and a single zero row of it
    _, gz, glz = run(ops, c, torch.zeros(B, T), **kw)
    assert bool((gz == 0).all()) and (glz is None or float(glz) == 0.0)
    g1 = c.gout.clone()
    live_row = int((~dead).nonzero()[0])
    g1[live_row] = 0
    _, gr, _ = run(ops, c, g1, **kw)
    assert bool((gr[live_row] == 0).all()) and bool(torch.isfinite(gr).all())
    others = torch.arange(B) != live_row
    assert torch.equal(gr[others.to(dev)], gq[others.to(dev)])


# ------------------------------------------------------------------------------------------------ 6. agreement with the class head
def test_one_hot_values_agree_with_the_class_head(ops, dev):
    c = case(ops, dev, SMALL, "euclidean")
    B, N, d, _ = SMALL
    onehot = F.one_hot(c.sy, C16).float()
    vals = ops.BankValues(onehot.to(dev), c.bank)
    target = torch.randint(0, C16, (B,), generator=torch.Generator().manual_seed(4))
    kw = c.variants["excluded single-row window"][0]
    keep = c.variants["excluded single-row window"][1]["keep"]
    rq, _ = c.ref(lambda out, rows: F.nll_loss(torch.log(out + 1e-12), target[rows], reduction="sum") / B, v=onehot, keep=keep)
    _, gq, _ = run(ops, c, loss=lambda out: F.nll_loss(out, target.to(dev)), vals=vals, log=True, **kw)
    close(gq, rq, "one-hot values, log, nll_loss")
    q = c.qd.clone().requires_grad_(True)
    F.nll_loss(ops.nw_head_bank(q, c.sd, c.sy.to(dev), C16, c.bank, **kw), target.to(dev)).backward()
    close(q.grad, rq, "nw_head_bank at the same inputs")


# ------------------------------------------------------------------------------------------------ 7. soft labels
@pytest.mark.parametrize("kind", ["euclidean", "cosine"])
def test_soft_labels_under_a_kl_loss(ops, dev, kind):
    c = case(ops, dev, SMALL, kind)
    B, N, d, _ = SMALL
    g = torch.Generator().manual_seed(12)
    soft = torch.softmax(2 * torch.randn(N, 10, generator=g), dim=1)
    target = torch.softmax(torch.randn(B, 10, generator=g), dim=1)
    vals = ops.BankValues(soft.to(dev), c.bank)
    kw, rkw = c.variants["weights"]
    rq, _ = c.ref(lambda out, rows: F.kl_div(torch.log(out + 1e-12), target[rows].double(), reduction="sum") / B, v=soft, **rkw)
    _, gq, _ = run(ops, c, loss=lambda out: F.kl_div(out, target.to(dev), reduction="batchmean"), vals=vals, log=True, **kw)
    close(gq, rq, f"soft labels, KL, {kind}")


# ------------------------------------------------------------------------------------------------ 8. constants and refusals
def test_constants_are_guarded_and_refusals_launch_nothing(ops, dev, launches):
    B, N, d, T = SMALL
    c = case(ops, dev, SMALL, "euclidean")
    sd, vd, a = c.sd.clone(), c.vd.clone(), torch.zeros(N, device=dev)
    bank = ops.SplitBank(sd, labels=c.sy.to(dev))
    vals = ops.BankValues(vd, bank)
    gout = c.gout.to(dev)

    def forward(**kw):
        q = c.qd.clone().requires_grad_(True)
        return q, ops.nw_head_values_bank(q, sd, bank, kw.pop("values", vals), row_logw=a, **kw)

    # the bank is written between forward and backward
    q, out = forward()
    bank.update_rows(sd, torch.tensor([3], device=dev), sd[5:6] * 0.5)
    n0 = len(launches)
    with pytest.raises(RuntimeError, match="bank was written"):
        out.backward(gout)
    assert len(launches) == n0 and q.grad is None
    # row_logw is written in place
    q, out = forward()
    a[7] = -1.0
    n0 = len(launches)
    with pytest.raises(RuntimeError, match="row_logw was written in place"):
        out.backward(gout)
    assert len(launches) == n0
    # the values' tensor is written: the BankValues has gone stale
    q, out = forward()
    vd[0, 0] += 1.0
    assert vals.stale()
    n0 = len(launches)
    with pytest.raises(RuntimeError, match="BankValues"):
        out.backward(gout)
    assert len(launches) == n0
    with pytest.raises(ValueError, match="written since"):           # ... and at the next forward
        forward()
    assert len(launches) == n0
    # an undisturbed step still runs
    vals = ops.BankValues(vd, bank)
    q, out = forward()
    out.backward(gout)
    assert launches[-1] == BWDV and bool(torch.isfinite(q.grad).all())
    # constants that require grad: refused on every route, nothing is detached silently
    fp16 = ops.SplitBank(sd, labels=c.sy.to(dev), precision="fp16")
    for bk in (bank, fp16):
        for kw in (dict(values=vd.clone().requires_grad_(True)), dict(values=ops.BankValues(vd.clone().requires_grad_(True), bk)),
                   dict(row_logw=a.clone().requires_grad_(True))):
            args = dict(values=vd, row_logw=a)
            args.update(kw)
            n0 = len(launches)
            with pytest.raises(ops.NWHipError, match="nw_scores"):
                ops.nw_head_values_bank(c.qd.clone().requires_grad_(True), sd, bk, args["values"], row_logw=args["row_logw"])
            assert len(launches) == n0
        n0 = len(launches)
        with pytest.raises(ValueError, match="requires grad"):
            ops.nw_head_values_bank(c.qd.clone().requires_grad_(True), sd.clone().requires_grad_(True), bk, vd)
        assert len(launches) == n0


# ------------------------------------------------------------------------------------------------ 9. the matrix route
def test_matrix_route(ops, dev, launches):
    B, N, d, T = SMALL
    for kind in ("euclidean", "clip"):
        c = case(ops, dev, SMALL, kind)
        kw, rkw = c.variants["window and weights"]
        rq, rls = c.parity_refs()["window and weights"]
        fp16 = ops.SplitBank(c.sd, labels=c.sy.to(dev), precision="fp16")
        del launches[:]
        q, ls = c.qd.clone().requires_grad_(True), c.ls()
        out = ops.nw_head_values_bank(q, c.sd, fp16, c.vd, kind, ls, **kw)
        out.backward(c.gout.to(dev))
        assert SCORES in launches and BWDV not in launches and VALUES not in launches, launches
        close(q.grad, rq, f"gq matrix route, fp16 bank, {kind}")
        if kind == "clip":
            close(ls.grad, rls, "gls matrix route, fp16 bank", ls=True)
        with torch.no_grad():
            assert torch.allclose(out.detach(), ops.nw_head_values(c.qd, c.sd, fp16, c.vd, kind, c.ls(False), **kw), rtol=1e-5, atol=1e-6)
    # N = 20, below the tile kernels; with dead queries (the kept window of rows that are switched off)
    for kind in KINDS:
        c = case(ops, dev, SMALL, kind)
        N2 = 20
        s2, v2 = c.s[:N2].contiguous(), c.v[:N2].contiguous()
        a2 = torch.tensor(PATTERN)[torch.arange(N2) % 7].clone()
        lo2, hi2 = torch.arange(B) % N2, torch.arange(B) % N2 + 1 + (torch.arange(B) % 3)
        keep2 = _admitted(N2, lo2, hi2, False)
        dead2 = ~(keep2 & torch.isfinite(a2)[None, :]).any(1)
        assert dead2.any() and not dead2.all()
        rq, rls = f64_grads(c.q, s2, v2, kind, {"x": dict(loss=dot_loss(c.gout), a=a2, keep=keep2)})["x"]
        s2d = s2.to(dev)
        del launches[:]
        q, ls = c.qd.clone().requires_grad_(True), c.ls()
        out = ops.nw_head_values_bank(q, s2d, ops.SplitBank(s2d), v2.to(dev), kind, ls, row_window=(lo2.to(dev), hi2.to(dev)),
                                      row_logw=a2.to(dev))
        out.backward(c.gout.to(dev))
        assert (SCORES in launches or PLAIN in launches) and BWDV not in launches and VALUES not in launches, launches
        close(q.grad, rq, f"gq matrix route, N = 20, {kind}")
        if kind == "clip":
            close(ls.grad, rls, "gls matrix route, N = 20", ls=True)
        assert bool((out.detach().cpu()[dead2] == 0).all()) and bool((q.grad.cpu()[dead2] == 0).all())


# ------------------------------------------------------------------------------------------------ 10. NWNet
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
    net = NWNet(torch.nn.Linear(48, 64), 10, support_dataset=DS(), n_shot_full=40, device=dev, **kw).to(dev)
    net.eval()
    with torch.no_grad():
        net.precompute()
    net.train()
    return net


def _net_ref(net, x, v, gout, leave_out=None, a=None):
    """fp64 gradients of sum(out * gout) w.r.t. the Linear featurizer's weight and bias, the bank as it stands."""
    from oracle import nw_oracle
    W = net.featurizer.weight.detach().cpu().double().requires_grad_(True)
    b = net.featurizer.bias.detach().cpu().double().requires_grad_(True)
    sc = nw_oracle.scores_f64(x.cpu().double() @ W.t() + b, net.full_feat.cpu(), "euclidean")
    keep = None
    if leave_out is not None:
        rows = leave_out.cpu()
        lo = rows.clamp(min=0)
        keep = _admitted(sc.shape[1], lo, torch.where(rows < 0, lo, lo + 1), True)
    out = weighted_mean_f64(sc, v.cpu(), a, keep)
    return torch.autograd.grad((out * gout.cpu().double()).sum(), (W, b))


def test_nwnet_forward_values(ops, dev, launches):
    net = _net(dev)
    N, T = net.full_feat.shape[0], 3
    g = torch.Generator().manual_seed(8)
    v = torch.randn(N, T, generator=g).to(dev)
    x = torch.randn(9, 48, generator=g).to(dev)
    gout = torch.randn(9, T, generator=g).to(dev)
    with pytest.raises(ops.NWHipError, match="forward_values: no values are set"):
        net.forward_values(x)
    net.set_support_values(v)
    rows = torch.tensor([3, -1, 399, 0, -1, 17, 200, 201, 40], device=dev)
    for leave_out in (None, rows):
        net.zero_grad()
        del launches[:]
        out = net.forward_values(x, leave_out=leave_out)
        assert out.shape == (9, T) and out.requires_grad and net.bank_features.shape == (9, 64) and not net.bank_features.requires_grad
        out.backward(gout)
        assert launches == [WINDOW, VALUES, BWDV]
        rw, rb = _net_ref(net, x, v, gout, leave_out)
        close(net.featurizer.weight.grad, rw, f"featurizer weight, leave_out {leave_out is not None}")
        close(net.featurizer.bias.grad, rb, f"featurizer bias, leave_out {leave_out is not None}")
    # log and return_mask
    logged = net.forward_values(x, log=True)
    assert torch.allclose(logged, torch.log(net.forward_values(x) + 1e-12), rtol=0, atol=0, equal_nan=True)
    net.return_mask = True
    out_m, mask = net.forward_values(x)
    assert out_m.shape == (9, T) and mask.shape == (9,) and bool(mask.all())
    net.return_mask = False
    # one cycle of memory-bank training: forward over the bank without the batch's own rows, backward, the rows refreshed
    own = torch.tensor([5, 44, 390, 128, 7, 260, 199, 81, 300], device=dev)
    net.zero_grad()
    net.forward_values(x, leave_out=own).backward(gout)
    before = net.full_feat[own].clone()
    net.refresh_bank(own)
    assert not torch.equal(net.full_feat[own], before) and net.support_values is not None
    net.zero_grad()
    del launches[:]
    net.forward_values(x, leave_out=own).backward(gout)
    assert launches == [WINDOW, VALUES, BWDV]
    rw, rb = _net_ref(net, x, v, gout, own)
    close(net.featurizer.weight.grad, rw, "featurizer weight over the refreshed bank")
    close(net.featurizer.bias.grad, rb, "featurizer bias over the refreshed bank")
    # support weights: a constant; learnable ones are read detached and receive no gradient
    a = _std_logw(net.full_y.cpu()).clamp(min=-5.0).to(dev)
    net.set_support_weights(a, learnable=True)
    net.zero_grad()
    del launches[:]
    net.forward_values(x, leave_out=own).backward(gout)
    assert launches == [WEIGHTED, VALUES, BWDV]
    assert net.support_logw.grad is None
    rw, rb = _net_ref(net, x, v, gout, own, a=a.cpu())
    close(net.featurizer.weight.grad, rw, "featurizer weight, learnable weights read detached")
    net.set_support_weights(None)
    # a sharded bank is refused
    net.sharded_bank = object()
    with pytest.raises(ops.NWHipError, match="sharded"):
        net.forward_values(x)
    net.sharded_bank = None
