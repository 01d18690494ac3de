"""The head's query gradient over a resident bank (bwd_query.hip: nw_bwd_query_f32, ops.nw_head_bank, NWNet.forward_bank)
against fp64 autograd of the oracle's head, rows masked before the softmax for windows.

Bar (the suite's bar for head gradients, test_head_backward_gpu.py): rtol = atol = 1e-4 on values divided by
max(|ref|.max(), 1e-3); logit_scale.grad: rtol 1e-4, atol 1e-6.  Every comparison prints its normalised error, and the
module prints the worst one at the end.
"""

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

KINDS = ("euclidean", "hypersphere_euclidean", "cosine", "dotproduct", "clip")
LS0 = float(np.log(1 / 0.07))
# ragged query and support tiles, d % 64 != 0, C beyond LDS; the last one is wider than the widest column slab (256)
SHAPES = [(64, 1024, 64, 5), (129, 257, 160, 1000), (33, 4099, 64, 7), (70, 1000, 544, 11)]
TILE_ROWS = 64      # bank rows per support tile of the kernel (bwd_query.hip, QBS)


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
    print(f"WORST bwd_query {WORST[0]:.3e} {WORST[1]}")


def nerr(got, ref):
    got, ref = got.detach().cpu().double().numpy(), ref.detach().double().numpy()
    return float(np.abs(got - ref).max()) / max(float(np.abs(ref).max()), 1e-3)


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


def head_f64(O, q, s, sy, C, kind, ls, keep=None):
    """fp64 head with `ls` in the graph; keep (B,N) bool: the rows each query's window admits."""
    if kind == "clip":
        qn = q / q.norm(dim=-1, keepdim=True).clamp_min(1e-12)
        sn = s / s.norm(dim=-1, keepdim=True).clamp_min(1e-12)
        sc = ls.exp() * (qn @ sn.t())
    else:
        sc = O.scores_f64(q, s, kind, LS0)
    if keep is not None:
        sc = sc.masked_fill(~keep, float("-inf"))
        live = keep.any(dim=1, keepdim=True)
        w = torch.where(live, torch.softmax(torch.where(live, sc, torch.zeros_like(sc)), dim=-1), torch.zeros_like(sc))
    else:
        w = torch.softmax(sc, dim=-1)
    return torch.log(w @ F.one_hot(sy, C).double() + 1e-12)


class Case:
    """Inputs of one (shape, kind), the bank on the device and fp64 reference gradients (computed once per loss)."""

    def __init__(self, O, ops, dev, B, N, d, C, kind, sort=False, n_labels=None):
        g = torch.Generator().manual_seed(B + N + d + C)
        self.O, self.shape, self.kind = O, (B, N, d, C), kind
        q0, s0 = torch.randn(B, d, generator=g), torch.randn(N, d, generator=g)
        if kind == "dotproduct":       # keep |score| O(1..10): the softmax of raw dot products is a one-hot otherwise
            q0, s0 = q0 * d ** -0.25, s0 * d ** -0.25
        self.q0, self.s0 = q0, s0
        self.sy = torch.randint(0, n_labels or C, (N,), generator=g)
        if sort:
            self.sy = self.sy.sort().values
        self.gen = g
        self.sd, self.syd = s0.to(dev), self.sy.to(dev)
        self.bank = ops.SplitBank(self.sd)
        self.memo = {}

    def ls(self, dev=None, grad=True):
        if self.kind != "clip":
            return None
        return torch.tensor(LS0, dtype=torch.float64 if dev is None else torch.float32, device=dev, requires_grad=grad)

    def ref(self, tag, gout, keep=None, q0=None):
        if tag not in self.memo:
            B, N, d, C = self.shape
            q = (self.q0 if q0 is None else q0).double().requires_grad_(True)
            ls = self.ls()
            out = head_f64(self.O, q, self.s0.double(), self.sy, C, self.kind, ls, keep)
            ins = (q,) + ((ls,) if ls is not None else ())
            gr = torch.autograd.grad((out * gout.double()).sum(), ins)
            self.memo[tag] = (gr[0], gr[1] if ls is not None else None)
        return self.memo[tag]


_CASES = {}


def case(O, ops, dev, shape, kind, **kw):
    key = (shape, kind, tuple(sorted(kw.items())))
    if key not in _CASES:
        _CASES[key] = Case(O, ops, dev, *shape, kind, **kw)
    return _CASES[key]


def run_bank(ops, c, dev, gout, window=None, exclude=False, q0=None):
    """(out, q.grad, logit_scale.grad) of ops.nw_head_bank under the upstream gradient `gout`."""
    q = (c.q0 if q0 is None else q0).to(dev).requires_grad_(True)
    ls = c.ls(dev)
    out = ops.nw_head_bank(q, c.sd, c.syd, c.shape[3], c.bank, c.kind, ls, row_window=window, exclude=exclude)
    out.backward(gout.to(dev))
    return out.detach(), q.grad, None if ls is None else ls.grad


def dense_gout(c, scale=1.0):
    B, _, _, C = c.shape
    return torch.randn(B, C, generator=torch.Generator().manual_seed(7)) * scale


# ------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_parity_with_fp64_and_with_the_parent_route(O, ops, dev, shape, kind):
    c = case(O, ops, dev, shape, kind)
    gout = dense_gout(c)
    out, gq, gls = run_bank(ops, c, dev, gout)
    rq, rls = c.ref("dense", gout)
    close(gq, rq, f"gq {kind} {shape}")
    if kind == "clip":
        close(gls, rls, f"gls {kind} {shape}", ls=True)
    # the forward is today's inference call, bit for bit
    with torch.no_grad():
        assert torch.equal(out, ops.nw_head(c.q0.to(dev), c.sd, c.syd, shape[3], kind, c.ls(dev, False), support_cache=c.bank))
    # the parent's route on the same inputs: nw_head through the score matrix
    q2 = c.q0.to(dev).requires_grad_(True)
    ops.nw_head(q2, c.sd, c.syd, shape[3], kind, c.ls(dev), support_cache=c.bank).backward(gout.to(dev))
    close(gq, q2.grad.cpu(), f"gq vs nw_head {kind} {shape}")


# ------------------------------------------------------------------------------------------------ chunks, workspace
def direct(c, dev, ops, gout, row_chunks=0, poison=None, window=None, exclude=False):
    """nw_bwd_query_f32 called directly with a workspace of the caller's (poison: byte to fill it with)."""
    from nwhead_amd import _lib
    lib = _lib.load()
    B, N, d, C = c.shape
    kid = ops.SCORE_KINDS[c.kind]
    q = c.q0.to(dev)
    ls = c.ls(dev, False)
    with torch.no_grad():
        if window is None:
            out, lse = torch.empty(B, C, device=dev), torch.empty(B, device=dev)
            fws = torch.empty(max(lib.nw_fwd_workspace_bytes(B, N, d, C), 1), dtype=torch.uint8, device=dev)
            _lib.check(lib.nw_fwd_f32(q.data_ptr(), c.sd.data_ptr(), c.syd.data_ptr(), c.bank.norm2.data_ptr(), c.bank.split.data_ptr(),
                                      c.bank.scale.data_ptr(), out.data_ptr(), None, lse.data_ptr(), None, fws.data_ptr(), fws.numel(),
                                      B, N, d, C, kid, None if ls is None else ls.data_ptr(), 0, 0, None, None), "nw_fwd_f32")
            lo = hi = None
        else:
            out, lse = ops.nw_head_window(q, c.sd, c.syd, C, c.bank, window, exclude, c.kind, ls, return_lse=True)
            lo, hi = (t.to(torch.int32).contiguous() for t in window)
    need = lib.nw_bwd_query_workspace_bytes(B, N, d, C, row_chunks)
    assert need > 0
    ws = torch.full((need,), 0 if poison is None else poison, dtype=torch.uint8, device=dev)
    gq = torch.empty(B, d, device=dev)
    gls = torch.empty((), device=dev)
    g = gout.to(dev).contiguous()
    _lib.check(lib.nw_bwd_query_f32(q.data_ptr(), c.bank.split.data_ptr(), c.bank.scale.data_ptr(), c.bank.norm2.data_ptr(),
                                    c.syd.data_ptr(), None if lo is None else lo.data_ptr(), None if hi is None else hi.data_ptr(),
                                    int(exclude), lse.data_ptr(), out.data_ptr(), g.data_ptr(), gq.data_ptr(), gls.data_ptr(),
                                    ws.data_ptr(), need, B, N, d, C, kid, None if ls is None else ls.data_ptr(), row_chunks, None),
               "nw_bwd_query_f32")
    torch.cuda.synchronize()
    return gq, gls


def test_chunk_reduction_is_deterministic_and_within_the_bar(O, ops, dev):
    shape = (33, 4099, 64, 7)
    c = case(O, ops, dev, shape, "euclidean")
    gout = dense_gout(c)
    rq, _ = c.ref("dense", gout)
    n_tiles = -(-shape[1] // TILE_ROWS)
    got = {}
    for rc in (1, 2, 3, 7, n_tiles, 10 * n_tiles):
        got[rc] = direct(c, dev, ops, gout, rc)[0]
        close(got[rc], rq, f"gq row_chunks={rc}")
        assert torch.equal(got[rc], direct(c, dev, ops, gout, rc)[0]), rc      # two calls: identical bits
    assert torch.equal(got[10 * n_tiles], got[n_tiles])                        # clamped to the tile count


@pytest.mark.parametrize("kind", ("euclidean", "clip"))
def test_poisoned_workspace_changes_nothing(O, ops, dev, kind):
    c = case(O, ops, dev, (33, 4099, 64, 7), kind)
    gout = dense_gout(c)
    for rc in (0, 3):
        a, b = direct(c, dev, ops, gout, rc), direct(c, dev, ops, gout, rc, poison=0xFF)
        assert torch.isfinite(b[0]).all()
        assert torch.equal(a[0], b[0]) and (kind != "clip" or torch.equal(a[1], b[1]))
    lo = torch.arange(33, device=dev) * 100
    win = (lo, lo + 700)
    a, b = direct(c, dev, ops, gout, 2, window=win), direct(c, dev, ops, gout, 2, poison=0xFF, window=win)
    assert torch.isfinite(b[0]).all() and torch.equal(a[0], b[0])


# ------------------------------------------------------------------------------------------------ windows
def keep_mask(lo, hi, N, exclude):
    cols = torch.arange(N)
    keep = (cols >= lo[:, None]) & (cols < hi[:, None])
    return ~keep if exclude else keep


@pytest.mark.parametrize("kind", ("euclidean", "cosine"))
def test_leave_one_out_of_the_banks_own_rows(O, ops, dev, kind):
    shape = (33, 4099, 64, 7)
    c = case(O, ops, dev, shape, kind)
    rows = torch.arange(33) * 123 + 5
    gout = dense_gout(c)
    q0 = c.s0[rows].clone()
    win = (rows.to(dev), (rows + 1).to(dev))
    _, gq, _ = run_bank(ops, c, dev, gout, win, True, q0=q0)
    rq, _ = c.ref("loo", gout, keep_mask(rows, rows + 1, shape[1], True), q0=q0)
    close(gq, rq, f"gq leave-one-out {kind}")
    # real rows and -1 mixed: -1 is the empty excluded window [0, 0)
    mixed = rows.clone()
    mixed[::3] = -1
    lo = mixed.clamp(min=0)
    hi = torch.where(mixed < 0, lo, lo + 1)
    _, gq, _ = run_bank(ops, c, dev, gout, (lo.to(dev), hi.to(dev)), True, q0=q0)
    rq, _ = c.ref("loo-mixed", gout, keep_mask(lo, hi, shape[1], True), q0=q0)
    close(gq, rq, f"gq leave-one-out with -1 {kind}")


def test_kept_window_of_one_class_and_an_empty_window(O, ops, dev):
    shape = (33, 4099, 64, 7)
    c = case(O, ops, dev, shape, "euclidean", sort=True)
    gout = dense_gout(c)
    cls = torch.arange(33) % 7
    lo = torch.searchsorted(c.sy, cls)
    hi = torch.searchsorted(c.sy, cls, right=True)
    lo[4], hi[4] = 17, 17                                   # a kept empty window: a dead query
    out, gq, _ = run_bank(ops, c, dev, gout, (lo.to(dev), hi.to(dev)), False)
    rq, _ = c.ref("one-class", gout, keep_mask(lo, hi, shape[1], False))
    close(gq, rq, "gq kept window of one class")
    assert torch.isfinite(out).all() and torch.isfinite(gq).all()
    assert not gq[4].any() and not rq[4].any()              # exactly zero


# ------------------------------------------------------------------------------------------------ absent classes
@pytest.mark.parametrize("kind", ("euclidean", "clip"))
def test_absent_class(O, ops, dev, kind):
    shape = (64, 1024, 64, 5)
    c = case(O, ops, dev, shape, kind, n_labels=4)          # no support carries class 4
    only = torch.zeros(64, 5)
    only[:, 4] = torch.randn(64, generator=torch.Generator().manual_seed(3))
    _, gq, gls = run_bank(ops, c, dev, only)
    assert not gq.any()                                     # exactly zero, bit for bit: t_b must not read the absent class
    assert gls is None or not gls.any()
    gout = dense_gout(c)
    _, gq, gls = run_bank(ops, c, dev, gout)
    rq, rls = c.ref("dense", gout)
    close(gq, rq, f"gq dense gout with an absent class {kind}")
    if kind == "clip":
        close(gls, rls, "gls dense gout with an absent class", ls=True)


# ------------------------------------------------------------------------------------------------ row weights
@pytest.mark.parametrize("kind", ("euclidean", "cosine"))
def test_row_weights(O, ops, dev, kind):
    shape = (64, 1024, 64, 5)
    c = case(O, ops, dev, shape, kind)
    gout = dense_gout(c, 1.0 / 64)
    _, base, _ = run_bank(ops, c, dev, gout)
    k = (torch.arange(64) % 41) - 20                        # 2^-20 .. 2^20
    w = torch.ldexp(torch.ones(64), k)
    w[5] = w[40] = 0.0
    _, gq, _ = run_bank(ops, c, dev, gout * w[:, None])
    assert torch.equal(gq, base * w.to(dev)[:, None])       # exactly scaled rows, exactly zero rows
    assert not gq[5].any() and not gq[40].any()
    # per-row weights spanning 2^+-10: every row normalised on its own (one exponent for the batch would fail the small rows)
    w = torch.ldexp(torch.ones(64), (torch.arange(64) % 21) - 10)
    _, gq, _ = run_bank(ops, c, dev, gout * w[:, None])
    rq, _ = c.ref("dense/64", gout)
    worst = max(nerr(gq[b:b + 1].cpu() / w[b], rq[b:b + 1]) for b in range(64))
    print(f"ERR {worst:.3e} rows normalised on their own {kind}")
    WORST[:] = max(WORST, [worst, f"row weights {kind}"], key=lambda t: t[0])
    for b in range(64):
        close(gq[b:b + 1].cpu() / w[b], rq[b:b + 1], f"row {b} of weight 2^{int(torch.log2(w[b]))} {kind}")


# ------------------------------------------------------------------------------------------------ memory
def test_no_score_matrix_is_allocated(O, ops, dev):
    B, N, d, C = 64, 65536, 64, 7
    g = torch.Generator().manual_seed(1)
    s = torch.randn(N, d, generator=g).to(dev)
    sy = (torch.arange(N) % C).sort().values.to(dev)
    q0 = torch.randn(B, d, generator=g).to(dev)
    t = torch.randint(0, C, (B,), generator=g).to(dev)
    bank = ops.SplitBank(s, labels=sy)
    matrix = B * N * 4

    def peak(fn):
        # The forward's scratch (nw_fwd_workspace_bytes: sized for whichever route the library takes, never below B N 4
        # bytes) is the process-wide buffer that every inference call of this shape already uses; it is warmed here like the
        # bank and is not part of what a training step allocates.  Everything the step itself needs is counted.
        ops._WS_CACHE.clear()
        with torch.no_grad():
            ops.nw_head(q0, s, sy, C, support_cache=bank)
        q = q0.clone().requires_grad_(True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        before = torch.cuda.memory_allocated(dev)
        F.nll_loss(fn(q), t).backward()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated(dev) - before, q.grad

    fused, g1 = peak(lambda q: ops.nw_head_bank(q, s, sy, C, bank))
    parent, g2 = peak(lambda q: ops.nw_head(q, s, sy, C, support_cache=bank))
    print(f"MEM nw_head_bank {fused} bytes, nw_head {parent} bytes, one score matrix {matrix} bytes")
    assert fused < matrix
    assert parent > 2 * matrix                               # the test can see the difference
    # both against fp64 at this size (the two routes differ from each other by the sum of their errors)
    q64 = q0.cpu().double().requires_grad_(True)
    ref = torch.autograd.grad(F.nll_loss(head_f64(O, q64, s.cpu().double(), sy.cpu(), C, "euclidean", None), t.cpu()), q64)[0]
    print(f"ERR {nerr(g2.cpu(), ref):.3e} nw_head's gq at 64 x 65536 x 64 (the route through the matrix, for comparison)")
    close(g1, ref, "gq at 64 x 65536 x 64")


# ------------------------------------------------------------------------------------------------ fallback
def test_banks_without_split_rows_fall_back_or_refuse(ops, dev):
    B, N, d, C = 32, 512, 64, 5
    g = torch.Generator().manual_seed(2)
    s, q0 = torch.randn(N, d, generator=g).to(dev), torch.randn(B, d, generator=g).to(dev)
    unsorted = torch.randint(0, C, (N,), generator=g).to(dev)
    gout = torch.randn(B, C, generator=g).to(dev)
    win = (torch.zeros(B, dtype=torch.int64, device=dev), torch.full((B,), 100, device=dev))
    for bank, sy in ((ops.SplitBank(s, precision="fp16"), unsorted.sort().values), (ops.SplitBank(s, labels=unsorted), unsorted)):
        q1, q2 = q0.clone().requires_grad_(True), q0.clone().requires_grad_(True)
        ops.nw_head_bank(q1, s, sy, C, bank).backward(gout)
        ops.nw_head(q2, s, sy, C, support_cache=bank).backward(gout)
        assert torch.equal(q1.grad, q2.grad)
        with pytest.raises(ops.NWHipError, match="no gradient route"):
            ops.nw_head_bank(q0.clone().requires_grad_(True), s, sy, C, bank, row_window=win)
    with pytest.raises(ValueError, match="constant"):
        ops.nw_head_bank(q0, s.clone().requires_grad_(True), unsorted, C, ops.SplitBank(s))


# ------------------------------------------------------------------------------------------------ NWNet.forward_bank
class _DS(torch.utils.data.Dataset):
    def __init__(self, data, targets, C):
        self.data, self.targets, self.num_classes = data, list(targets), C

    def __len__(self):
        return len(self.targets)

    def __getitem__(self, i):
        return self.data[i], self.targets[i]


@pytest.mark.parametrize("leave", (False, True))
def test_nwnet_forward_bank(O, dev, leave):
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
    assert N == C * n and net.full_cache.split is not None and net.full_cache.sorted_rows is None
    B = 24
    x = torch.randn(B, din, generator=g)
    rows = torch.randint(0, N, (B,), generator=g)
    rows[::4] = -1
    gout = torch.randn(B, C, generator=g)
    lo = rows.clamp(min=0)
    keep = keep_mask(lo, torch.where(rows < 0, lo, lo + 1), N, True) if leave else None
    leave_out = rows.to(dev) if leave else None
    # reference: fp64 autograd through the same Linear over the bank as a constant
    W = feat.weight.detach().cpu().double().requires_grad_(True)
    b = feat.bias.detach().cpu().double().requires_grad_(True)
    ref = head_f64(O, x.double() @ W.t() + b, net.full_feat.cpu().double(), net.full_y.cpu(), C, "euclidean", None, keep)
    rW, rb = torch.autograd.grad((ref * gout.double()).sum(), (W, b))
    net.zero_grad()
    out = net.forward_bank(x.to(dev), leave_out=leave_out)
    out.backward(gout.to(dev))
    close(feat.weight.grad, rW, f"forward_bank weight.grad leave_out={leave}")
    close(feat.bias.grad, rb, f"forward_bank bias.grad leave_out={leave}")
    with torch.no_grad():
        assert torch.equal(net.forward_bank(x.to(dev), leave_out=leave_out), net.predict(x.to(dev), "full", leave_out=leave_out))
        assert torch.equal(out.detach(), net.predict(x.to(dev), "full", leave_out=leave_out))
    net.return_mask = True
    o2, mask = net.forward_bank(x.to(dev), leave_out=leave_out)
    assert torch.equal(o2.detach(), out.detach()) and mask.shape == (B,) and bool(mask.all())
