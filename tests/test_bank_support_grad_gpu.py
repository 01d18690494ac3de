"""The head's gradient to the BANK ROWS over a resident bank (bwd_support.hip: nw_bwd_bank_support_f32,
ops.nw_head_bank(support_grad=True), ops.SplitBank.refresh, NWNet.set_bank_learnable) against fp64 torch autograd of the
oracle's head with `s` a leaf, rows masked before the softmax and dead queries 0.

Bar (the suite's bar for head gradients, test_bwd_query_gpu.py): rtol = atol = 1e-4 on values divided by
max(|ref|.max(), 1e-3).  Every comparison prints its normalised error, and the module prints the worst one at the end
(DESIGN.md 4.6d).
"""

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

KINDS = ("euclidean", "hypersphere_euclidean", "cosine", "dotproduct", "clip")
LS0 = float(np.log(1 / 0.07))
# ragged query, support and column tiles, a padded width (160 -> 192), more than one column slab (544 > 256), C beyond a tile
SHAPES = [(64, 1024, 64, 5), (129, 257, 160, 1000), (33, 4099, 64, 7), (70, 1000, 544, 11)]
INF = float("inf")


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


WORST = [0.0, ""]


@pytest.fixture(scope="module", autouse=True)
def report_worst():
    yield
    _CASES.clear()
    print(f"WORST bank_support {WORST[0]:.3e} {WORST[1]}")


def close(got, ref, what):
    got, ref = got.detach().cpu().double().numpy(), ref.detach().cpu().double().numpy()
    assert np.isfinite(got).all() and np.isfinite(ref).all(), what
    scale = max(float(np.abs(ref).max()), 1e-3)
    err = float(np.abs(got - ref).max()) / scale
    if err > WORST[0]:
        WORST[:] = [err, what]
    print(f"ERR {err:.3e} {what}")
    np.testing.assert_allclose(got / scale, ref / scale, rtol=1e-4, atol=1e-4, err_msg=what)


def head_f64(O, q, s, sy, C, kind, ls, keep=None, logw=None):
    """fp64 head; keep (B,N) bool: the rows each query's window admits; logw (N,): log-weights, -inf removes a row."""
    if kind == "clip":
        qn = q / q.norm(dim=-1, keepdim=True).clamp_min(1e-12)
        sn = s / s.norm(dim=-1, keepdim=True).clamp_min(1e-12)
        sc = ls.exp() * (qn @ sn.t())
    elif kind in ("euclidean", "hypersphere_euclidean"):
        # scores_f64's values; its sqrt has the gradient 0 / 0 at a distance of exactly 0 (a query that is a bank row, a zero
        # query against a zero row), where torch.cdist, backward.hip and the kernels pass no gradient: that convention here
        xq, sx = q[:, None, :], s[None]
        if kind == "hypersphere_euclidean":
            xq = xq / xq.norm(dim=-1, keepdim=True).clamp_min(1e-12)
            sx = sx / sx.norm(dim=-1, keepdim=True).clamp_min(1e-12)
        d2 = (xq - sx).pow(2).sum(-1)
        sc = -torch.where(d2 > 0, torch.where(d2 > 0, d2, torch.ones_like(d2)).sqrt(), torch.zeros_like(d2))
        assert torch.equal(sc.detach(), O.scores_f64(q.detach(), s.detach(), kind, LS0))
    else:
        sc = O.scores_f64(q, s, kind, LS0)
    if logw is not None:
        a = logw.double()
        on = (a > -INF)[None, :].expand_as(sc)
        keep = on if keep is None else keep & on
        sc = sc + torch.where(a > -INF, a, torch.zeros_like(a))
    if keep is not None:
        sc = sc.masked_fill(~keep, -INF)
        live = keep.any(dim=1, keepdim=True)
        w = torch.where(live, torch.softmax(torch.where(live, sc, torch.zeros_like(sc)), dim=-1), torch.zeros_like(sc))
    else:
        w = torch.softmax(sc, dim=-1)
    return torch.log(w @ F.one_hot(sy, C).double() + 1e-12)


class Case:
    """Inputs of one (shape, kind), the bank on the device and fp64 reference gradients (computed once per tag)."""

    def __init__(self, O, ops, dev, B, N, d, C, kind, sort=False, zero=False):
        g = torch.Generator().manual_seed(B + N + d + C)
        self.O, self.shape, self.kind = O, (B, N, d, C), kind
        q0, s0 = torch.randn(B, d, generator=g), torch.randn(N, d, generator=g)
        if kind == "dotproduct":       # keep |score| O(1..10): the softmax of raw dot products is a one-hot otherwise
            q0, s0 = q0 * d ** -0.25, s0 * d ** -0.25
        if zero:                       # one all-zero bank row and one all-zero query
            s0[N // 3] = 0.0
            q0[B // 2] = 0.0
        self.q0, self.s0 = q0, s0
        self.sy = torch.randint(0, C, (N,), generator=g)
        if sort:
            self.sy = self.sy.sort().values
        self.sd, self.syd = s0.to(dev), self.sy.to(dev)
        self.bank = ops.SplitBank(self.sd)
        self.memo = {}

    def ls(self, dev=None, grad=False):
        if self.kind != "clip":
            return None
        return torch.tensor(LS0, dtype=torch.float64 if dev is None else torch.float32, device=dev, requires_grad=grad)

    def ref(self, tag, gout, keep=None, logw=None, q0=None):
        """fp64 (gs, gq) under the upstream gradient gout."""
        if tag not in self.memo:
            C = self.shape[3]
            q = (self.q0 if q0 is None else q0).double().requires_grad_(True)
            s = self.s0.double().requires_grad_(True)
            out = head_f64(self.O, q, s, self.sy, C, self.kind, self.ls(), keep, logw)
            gs, gq = torch.autograd.grad((out * gout.double()).sum(), (s, q))
            self.memo[tag] = (gs, gq)
        return self.memo[tag]


_CASES = {}


def case(O, ops, dev, shape, kind, **kw):
    key = (shape, kind, tuple(sorted(kw.items())))
    if key not in _CASES:
        _CASES[key] = Case(O, ops, dev, *shape, kind, **kw)
    return _CASES[key]


def dense_gout(c, scale=1.0):
    B, _, _, C = c.shape
    return torch.randn(B, C, generator=torch.Generator().manual_seed(7)) * scale


def run_bank(ops, c, dev, gout, window=None, exclude=False, q0=None, logw=None, q_grad=False):
    """(out, s.grad, q.grad) of ops.nw_head_bank(support_grad=True) under the upstream gradient `gout`; the bank's own
    tensor is the leaf (the bank matches it by address, shape and version)."""
    q = (c.q0 if q0 is None else q0).to(dev).requires_grad_(q_grad)
    s = c.sd.requires_grad_(True)
    s.grad = None
    try:
        out = ops.nw_head_bank(q, s, c.syd, c.shape[3], c.bank, c.kind, c.ls(dev), row_window=window, exclude=exclude,
                               row_logw=None if logw is None else logw.to(dev), support_grad=True)
        out.backward(gout.to(dev))
        return out.detach(), s.grad, q.grad
    finally:
        s.requires_grad_(False)
        s.grad = None


# ------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_parity_with_fp64_and_with_the_parent_route(O, ops, dev, shape, kind):
    c = case(O, ops, dev, shape, kind)
    B, N, d, C = shape
    gout = dense_gout(c)
    out, gs, gq = run_bank(ops, c, dev, gout, q_grad=True)
    rs, rq = c.ref("dense", gout)
    assert gs.shape == (N, d) and gs.dtype == torch.float32
    close(gs, rs, f"gs {kind} {shape}")
    # the forward is today's inference call, bit for bit
    with torch.no_grad():
        assert torch.equal(out, ops.nw_head(c.q0.to(dev), c.sd, c.syd, C, kind, c.ls(dev), support_cache=c.bank))
    # gq beside gs: the bits of the call without the keyword
    q1 = c.q0.to(dev).requires_grad_(True)
    ops.nw_head_bank(q1, c.sd, c.syd, C, c.bank, kind, c.ls(dev)).backward(gout.to(dev))
    assert torch.equal(gq, q1.grad)
    # only the rows learning: the same gs
    _, gs_only, none = run_bank(ops, c, dev, gout)
    assert none is None and torch.equal(gs_only, gs)
    # the parent's route on the same inputs: nw_head through the score matrix
    s2 = c.sd.clone().requires_grad_(True)
    ops.nw_head(c.q0.to(dev), s2, c.syd, C, kind, c.ls(dev)).backward(gout.to(dev))
    close(gs, s2.grad, f"gs vs nw_head {kind} {shape}")


def test_only_the_rows_learning_makes_no_query_gradient_call(O, ops, dev, monkeypatch):
    c = case(O, ops, dev, (64, 1024, 64, 5), "euclidean")
    calls = []
    real = ops._bank_head_bwd
    monkeypatch.setattr(ops, "_bank_head_bwd", lambda *a, **k: calls.append(1) or real(*a, **k))
    run_bank(ops, c, dev, dense_gout(c))
    assert not calls
    run_bank(ops, c, dev, dense_gout(c), q_grad=True)
    assert len(calls) == 1


def test_default_keyword_still_refuses_a_support_that_requires_grad(ops, dev):
    s = torch.randn(100, 64, device=dev)
    bank = ops.SplitBank(s)
    sy = torch.zeros(100, dtype=torch.int64, device=dev)
    with pytest.raises(ValueError, match="the bank is a constant here"):
        ops.nw_head_bank(torch.randn(4, 64, device=dev), s.requires_grad_(True), sy, 2, bank)


# ------------------------------------------------------------------------------------------------ windows and weights
def keep_mask(lo, hi, N, exclude):
    cols = torch.arange(N)
    keep = (cols >= lo[:, None]) & (cols < hi[:, None])
    return ~keep if exclude else keep


def nobody(keep, logw=None):
    """(N,) bool: the rows no query admits or that sit at -inf."""
    dead = ~keep.any(dim=0) if keep is not None else torch.zeros(logw.shape[0], dtype=torch.bool)
    return dead | (logw == -INF) if logw is not None else dead


@pytest.mark.parametrize("kind", ("euclidean", "cosine"))
def test_leave_one_out_of_the_banks_own_rows(O, ops, dev, kind):
    shape = (33, 4099, 64, 7)
    c = case(O, ops, dev, shape, kind)
    rows = torch.arange(33) * 123 + 5
    rows[::3] = -1                                           # -1 is the empty excluded window [0, 0)
    gout = dense_gout(c)
    # a query that leaves its row out IS that row; one with -1 is a sample the bank does not hold.  (A copy of a row that is
    # NOT left out sits at a distance of exactly 0, where the reference passes no gradient by convention and 1 / D of the
    # recomputed fp32 distance is noise: no such pair here.)
    q0 = torch.where((rows >= 0)[:, None], c.s0[rows.clamp(min=0)], c.q0)
    lo = rows.clamp(min=0)
    hi = torch.where(rows < 0, lo, lo + 1)
    _, gs, _ = run_bank(ops, c, dev, gout, (lo.to(dev), hi.to(dev)), True, q0=q0)
    rs, _ = c.ref("loo", gout, keep_mask(lo, hi, shape[1], True), q0=q0)
    close(gs, rs, f"gs leave-one-out with -1 {kind}")


@pytest.mark.parametrize("kind", ("euclidean", "cosine"))
def test_kept_window_of_one_class_an_empty_window_and_rows_nobody_admits(O, ops, dev, kind):
    shape = (33, 4099, 64, 7)
    c = case(O, ops, dev, shape, kind, sort=True)
    gout = dense_gout(c)
    cls = torch.arange(33) % 5                               # classes 5 and 6: rows that nobody admits
    lo = torch.searchsorted(c.sy, cls)
    hi = torch.searchsorted(c.sy, cls, right=True)
    lo[4], hi[4] = 17, 17                                    # a kept empty window: a dead query
    keep = keep_mask(lo, hi, shape[1], False)
    _, gs, _ = run_bank(ops, c, dev, gout, (lo.to(dev), hi.to(dev)), False)
    rs, _ = c.ref("one-class", gout, keep)
    close(gs, rs, f"gs kept window of one class {kind}")
    dead = nobody(keep)
    assert int(dead.sum()) > 64 and bool((gs.cpu()[dead] == 0.0).all()) and bool((rs[dead] == 0.0).all())


@pytest.mark.parametrize("kind", ("euclidean", "cosine"))
def test_row_weights_with_and_without_a_window(O, ops, dev, kind):
    shape = (33, 4099, 64, 7)
    c = case(O, ops, dev, shape, kind)
    N = shape[1]
    g = torch.Generator().manual_seed(9)
    logw = torch.randn(N, generator=g)
    logw[torch.randperm(N, generator=g)[:300]] = -INF
    logw[64:128] = -INF                                      # a whole support tile at -inf
    gout = dense_gout(c)
    _, gs, _ = run_bank(ops, c, dev, gout, logw=logw)
    rs, _ = c.ref("weights", gout, logw=logw)
    close(gs, rs, f"gs row weights {kind}")
    off = logw == -INF
    assert bool((gs.cpu()[off] == 0.0).all())
    # a window and weights together
    lo = (torch.arange(33) * 100) % N
    hi = lo + 700
    keep = keep_mask(lo, hi, N, False)
    _, gs, _ = run_bank(ops, c, dev, gout, (lo.to(dev), hi.to(dev)), False, logw=logw)
    rs, _ = c.ref("weights+window", gout, keep, logw=logw)
    close(gs, rs, f"gs row weights and a window {kind}")
    dead = nobody(keep, logw)
    assert bool((gs.cpu()[dead] == 0.0).all()) and bool((rs[dead] == 0.0).all())


@pytest.mark.parametrize("kind", ("euclidean", "hypersphere_euclidean"))
def test_distance_derivative_takes_the_raw_score(O, ops, dev, kind):
    """a = +3 on a near row: with the weighted score in the distance's place 1 / D is off by far more than the bar."""
    shape = (64, 1024, 64, 5)
    c = case(O, ops, dev, shape, kind)
    q0 = c.q0.clone()
    q0[3] = c.s0[100] + 0.05 * torch.randn(64, generator=torch.Generator().manual_seed(4))      # a near row
    logw = torch.zeros(shape[1])
    logw[100] = 3.0
    gout = dense_gout(c)
    _, gs, _ = run_bank(ops, c, dev, gout, q0=q0, logw=logw)
    rs, _ = c.ref("raw-score", gout, logw=logw, q0=q0)
    close(gs, rs, f"gs with a = +3 on a near row {kind}")
    close(gs[100:101], rs[100:101], f"gs of the near row itself {kind}")


# ------------------------------------------------------------------------------------------------ degenerate rows
@pytest.mark.parametrize("kind", KINDS)
def test_an_all_zero_bank_row_and_an_all_zero_query(O, ops, dev, kind):
    shape = (64, 1024, 64, 5)
    c = case(O, ops, dev, shape, kind, zero=True)
    gout = dense_gout(c)
    _, gs, _ = run_bank(ops, c, dev, gout)
    rs, _ = c.ref("dense", gout)
    close(gs, rs, f"gs zero row and zero query {kind}")
    # The other rows on their own scale.  The normalising kinds give the zero row a gradient of the order 1 / 1e-12 (so does
    # the reference), which is the scale of the comparison above; the workgroup's exponent follows it, and the 63 rows that
    # share its support tile keep only what lies within 2^-40 of it: they are left out here.
    other = torch.ones(shape[1], dtype=torch.bool)
    z = shape[1] // 3
    if kind in ("euclidean", "dotproduct"):
        other[z] = False
    else:
        other[z // 64 * 64:z // 64 * 64 + 64] = False
    close(gs[other], rs[other], f"gs of the other rows, zero row and zero query {kind}")


# ------------------------------------------------------------------------------------------------ direct calls
def direct(c, dev, ops, gout, query_chunks=0, poison=None, window=None, exclude=False):
    """nw_bwd_bank_support_f32 called directly with a workspace of the caller's (poison: byte to fill it with) -> gs at the
    bank's (padded) width."""
    from nwhead_amd import _lib
    lib = _lib.load()
    B, N, _, C = c.shape
    kid = ops.SCORE_KINDS[c.kind]
    call = ops._resolve_scores(c.bank, c.q0.to(dev))
    q, d = call.q.contiguous(), c.bank.shape[1]
    rows = c.bank.rows if c.bank.rows is not None else c.sd
    ls = c.ls(dev)
    whole = (torch.zeros(B, dtype=torch.int64, device=dev), torch.full((B,), N, dtype=torch.int64, device=dev))
    with torch.no_grad():
        out, lse = ops.nw_head_window(c.q0.to(dev), c.sd, c.syd, C, c.bank, window or whole, exclude, c.kind, ls, return_lse=True)
    lo, hi = (t.to(torch.int32).contiguous() for t in window) if window is not None else (None, None)
    need = lib.nw_bwd_bank_support_workspace_bytes(B, N, d, C, query_chunks)
    assert need > 0
    ws = torch.full((need,), 0 if poison is None else poison, dtype=torch.uint8, device=dev)
    gs = torch.empty(N, d, device=dev)
    g = gout.to(dev).contiguous()
    _lib.check(lib.nw_bwd_bank_support_f32(q.data_ptr(), rows.data_ptr(), c.bank.split.data_ptr(), c.bank.scale.data_ptr(),
                                           c.bank.norm2.data_ptr(), c.syd.data_ptr(), None, None if lo is None else lo.data_ptr(),
                                           None if hi is None else hi.data_ptr(), int(exclude), lse.data_ptr(), out.data_ptr(),
                                           g.data_ptr(), gs.data_ptr(), ws.data_ptr(), need, B, N, d, C, kid,
                                           None if ls is None else ls.data_ptr(), query_chunks, None), "nw_bwd_bank_support_f32")
    torch.cuda.synchronize()
    return gs


@pytest.mark.parametrize("shape", [(129, 257, 160, 1000), (300, 200, 64, 5)], ids=lambda s: "x".join(map(str, s)))
def test_query_chunks_are_deterministic_and_within_the_bar(O, ops, dev, shape):
    c = case(O, ops, dev, shape, "euclidean")
    gout = dense_gout(c)
    rs, _ = c.ref("dense", gout)
    n_qtiles = -(-shape[0] // 64)
    for qc in sorted({1, 2, 3, n_qtiles}):
        gs = direct(c, dev, ops, gout, qc)
        close(gs[:, :shape[2]], rs, f"gs query_chunks={qc} {shape}")
        assert not gs[:, shape[2]:].any()                                       # the zero columns of a padded bank
        assert torch.equal(gs, direct(c, dev, ops, gout, qc)), qc               # two calls: identical bits


@pytest.mark.parametrize("kind", ("euclidean", "clip"))
def test_poisoned_workspace_changes_nothing(O, ops, dev, kind):
    c = case(O, ops, dev, (129, 257, 160, 1000), kind)
    gout = dense_gout(c)
    for qc in (0, 1, 2):
        a, b = direct(c, dev, ops, gout, qc), direct(c, dev, ops, gout, qc, poison=0xFF)
        assert torch.isfinite(b).all() and torch.equal(a, b)
    lo = torch.arange(129, device=dev) % 100
    win = (lo, lo + 150)
    a, b = direct(c, dev, ops, gout, 2, window=win), direct(c, dev, ops, gout, 2, poison=0xFF, window=win)
    assert torch.isfinite(b).all() and torch.equal(a, b)


@pytest.mark.parametrize("kind", ("euclidean", "cosine"))
def test_gout_times_a_power_of_two_scales_gs_exactly(O, ops, dev, kind):
    c = case(O, ops, dev, (129, 257, 160, 1000), kind)
    gout = dense_gout(c)
    base = direct(c, dev, ops, gout, 2)
    for k in (-20, -3, 7, 20):
        assert torch.equal(direct(c, dev, ops, gout * 2.0 ** k, 2), base * 2.0 ** k), k


# ------------------------------------------------------------------------------------------------ memory
def test_no_score_matrix_is_allocated(O, ops, dev):
    B, N, d, C = 256, 32768, 64, 7
    g = torch.Generator().manual_seed(1)
    s = torch.randn(N, d, generator=g).to(dev)
    sy = (torch.arange(N) % C).sort().values.to(dev)
    q = torch.randn(B, d, generator=g).to(dev)
    t = torch.randint(0, C, (B,), generator=g).to(dev)
    bank = ops.SplitBank(s, labels=sy)
    matrix = B * N * 4

    def peak(fn):
        # the forward's scratch and the backward's workspace are process-wide buffers that are only ever grown: they are
        # warmed by a first step and are not part of what a later step allocates; gs itself is the result
        for _ in range(2):
            s.grad = None
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(dev)
            before = torch.cuda.memory_allocated(dev)
            F.nll_loss(fn(s.requires_grad_(True)), t).backward()
            torch.cuda.synchronize()
            used = torch.cuda.max_memory_allocated(dev) - before
        grad = s.grad
        s.requires_grad_(False)
        s.grad = None
        return used - N * d * 4, grad

    fused, g1 = peak(lambda sp: ops.nw_head_bank(q, sp, sy, C, bank, support_grad=True))
    parent, g2 = peak(lambda sp: ops.nw_head(q, sp, sy, C, support_cache=bank))
    print(f"MEM nw_head_bank(support_grad=True) {fused} bytes beyond gs, nw_head {parent} bytes, one score matrix {matrix} bytes")
    assert fused < matrix
    assert parent > matrix                                   # the test can see the difference
    s64 = s.cpu().double().requires_grad_(True)
    ref = torch.autograd.grad(F.nll_loss(head_f64(O, q.cpu().double(), s64, sy.cpu(), C, "euclidean", None), t.cpu()), s64)[0]
    close(g1, ref, "gs at 256 x 32768 x 64 under nll_loss")


# ------------------------------------------------------------------------------------------------ SplitBank.refresh
@pytest.mark.parametrize("d,precision", [(64, "fp32"), (160, "fp32"), (64, "fp16"), (100, "fp16")])
def test_refresh_equals_a_fresh_bank_bit_for_bit(ops, dev, d, precision):
    g = torch.Generator().manual_seed(d)
    N = 300
    s = torch.randn(N, d, generator=g).to(dev)
    sy = (torch.arange(N) % 5).sort().values.to(dev)
    bank = ops.SplitBank(s, labels=sy, precision=precision)
    names = ("rows", "split", "scale", "norm2", "packed", "packed_scale", "packed_norm2")
    ptrs = {n: getattr(bank, n).data_ptr() for n in names if getattr(bank, n) is not None}
    tables, writes = bank.tables, bank.writes
    s.copy_(torch.randn(N, d, generator=g) * 3.0)            # an in-place write of all rows
    assert not bank.matches(s)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    bank.refresh(s)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated(dev) == before    # no allocation
    assert bank.matches(s) and bank.writes == writes + 1 and bank.tables is tables
    fresh = ops.SplitBank(s, labels=sy, precision=precision)
    for n in names:
        a, b = getattr(bank, n), getattr(fresh, n)
        assert (a is None) == (b is None), n
        if a is not None:
            assert torch.equal(a, b), n
            assert a.data_ptr() == ptrs[n], n
    assert (bank.pad, bank.shape) == (fresh.pad, fresh.shape)


def test_refresh_refuses_a_class_sorted_copy_and_another_shape(ops, dev):
    s = torch.randn(200, 64, device=dev)
    unsorted = torch.randint(0, 5, (200,), device=dev)
    with pytest.raises(ops.NWHipError, match="class-sorted copy"):
        ops.SplitBank(s, labels=unsorted).refresh(s)
    with pytest.raises(ValueError, match="refresh"):
        ops.SplitBank(s).refresh(s[:100])


def test_a_backward_after_refresh_is_refused(ops, dev):
    s = torch.randn(200, 64, device=dev).requires_grad_(True)
    sy = torch.randint(0, 5, (200,), device=dev)
    bank = ops.SplitBank(s)
    out = ops.nw_head_bank(torch.randn(8, 64, device=dev), s, sy, 5, bank, support_grad=True)
    bank.refresh(s)
    with pytest.raises(RuntimeError, match="the bank was written"):
        out.sum().backward()


# ------------------------------------------------------------------------------------------------ fallbacks
def test_banks_without_split_rows_fall_back_or_refuse(O, ops, dev):
    B, N, d, C = 32, 512, 64, 5
    g = torch.Generator().manual_seed(2)
    s0, q0 = torch.randn(N, d, generator=g), torch.randn(B, d, generator=g)
    unsorted = torch.randint(0, C, (N,), generator=g)
    gout = torch.randn(B, C, generator=g)
    banks = [("fp16", N, lambda s, sy: ops.SplitBank(s, precision="fp16"), True),
             ("unsorted labels", N, lambda s, sy: ops.SplitBank(s, labels=sy), False),
             ("N <= 25", 20, lambda s, sy: ops.SplitBank(s), True)]
    for name, n, build, sort in banks:
        sy = unsorted[:n].sort().values if sort else unsorted[:n]
        s = s0[:n].to(dev).requires_grad_(True)
        bank = build(s, sy.to(dev))
        ops.nw_head_bank(q0.to(dev), s, sy.to(dev), C, bank, support_grad=True).backward(gout.to(dev))
        s64 = s0[:n].double().requires_grad_(True)
        ref = torch.autograd.grad((head_f64(O, q0.double(), s64, sy, C, "euclidean", None) * gout.double()).sum(), s64)[0]
        close(s.grad, ref, f"gs on the matrix route: {name}")
        win = (torch.zeros(B, dtype=torch.int64, device=dev), torch.full((B,), 10, device=dev))
        with pytest.raises(ops.NWHipError, match="no gradient route"):
            ops.nw_head_bank(q0.to(dev), s, sy.to(dev), C, bank, row_window=win, support_grad=True)
        with pytest.raises(ops.NWHipError, match="no gradient route"):
            ops.nw_head_bank(q0.to(dev), s, sy.to(dev), C, bank, row_logw=torch.zeros(n, device=dev), support_grad=True)


# ------------------------------------------------------------------------------------------------ NWNet.set_bank_learnable
class _DS(torch.utils.data.Dataset):
    def __init__(self, data, targets, C):
        self.data, self.targets, self.num_classes = data, list(targets), C

    def __len__(self):
        return len(self.targets)

    def __getitem__(self, i):
        return self.data[i], self.targets[i]


def test_nwnet_learnable_bank(O, dev):
    from nwhead_amd import ops
    from nwhead_amd.nwhead.nw import NWNet
    g = torch.Generator().manual_seed(5)
    C, n, din, d = 6, 40, 48, 64
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
    assert "support_bank" not in dict(net.named_parameters())
    net.set_bank_learnable()
    assert "support_bank" in dict(net.named_parameters()) and "support_bank" in net.state_dict()
    assert net.support_bank.data_ptr() == net.full_feat.data_ptr() and net.support_bank.requires_grad
    B = 24
    x = torch.randn(B, din, generator=g)
    rows = torch.randint(0, N, (B,), generator=g)
    rows[::4] = -1
    gout = torch.randn(B, C, generator=g)
    lo = rows.clamp(min=0)
    keep = keep_mask(lo, torch.where(rows < 0, lo, lo + 1), N, True)
    W, b = feat.weight.detach().cpu().double(), feat.bias.detach().cpu().double()
    s64 = net.full_feat.detach().cpu().double().requires_grad_(True)
    ref = head_f64(O, x.double() @ W.t() + b, s64, net.full_y.cpu(), C, "euclidean", None, keep)
    rs = torch.autograd.grad((ref * gout.double()).sum(), s64)[0]
    net.zero_grad()
    cache, ptr = net.full_cache, net.full_cache.split.data_ptr()
    out = net.forward_bank(x.to(dev), leave_out=rows.to(dev))
    out.backward(gout.to(dev))
    close(net.support_bank.grad, rs, "support_bank.grad, forward_bank with leave_out")
    assert feat.weight.grad is not None
    # an optimizer step on the rows: the next calls read the bank re-prepared in place, bit for bit a freshly built one
    torch.optim.SGD([net.support_bank], lr=0.5).step()
    with torch.no_grad():
        again = net.forward_bank(x.to(dev))
        full = net.predict(x.to(dev), "full")
        assert net.full_cache is cache and cache.split.data_ptr() == ptr and cache.matches(net.full_feat)
        fresh = ops.SplitBank(net.full_feat.detach().clone(), labels=net.full_y)
        assert torch.equal(cache.split, fresh.split) and torch.equal(cache.norm2, fresh.norm2)
        s2 = net.full_feat.detach().clone()
        want = ops.nw_head(net.featurizer(x.to(dev)), s2, net.full_y, C, "euclidean", None, support_cache=ops.SplitBank(s2, labels=net.full_y))
        assert torch.equal(again, want) and torch.equal(full, want)
        assert not torch.equal(again, out.detach())
    net.set_bank_learnable(False)
    assert "support_bank" not in dict(net.named_parameters())
    net.set_bank_learnable()
    net.precompute()
    assert "support_bank" not in dict(net.named_parameters()) and "support_bank" not in net.state_dict()
