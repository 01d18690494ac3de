"""Support weights in the fused head: ops.nw_head / nw_head_window / nw_head_bank(row_logw=...) -> nw_fwd_weighted_f32 and
nw_bwd_query_weighted_f32.  A log-weight a_j per bank row is added to the score in the tile epilogue BEFORE the masks and the
tile maximum (fused_impl.h, OUT_WGT), and in the query gradient it enters the softmax weight W alone (bwd_query.hip, WGT).

Reference: fp64 torch on the CPU, log(softmax(score + a over the admitted rows) @ one_hot + 1e-12), dead queries (no admitted
row with a finite weight) set to log(1e-12); gradients by autograd through the same expression.
Forward tolerance: the bank-path bound of test_head_window_gpu.py, rtol 1e-5 and atol max(3e-5, 3e-6 * smax) with
smax = max |score + a| over the finite entries (the magnitude the kernel's exponent argument carries).
Gradient tolerance: the bar of test_bwd_query_gpu.py, rtol = atol = 1e-4 on values divided by max(|ref|.max(), 1e-3);
logit_scale.grad rtol 1e-4, atol 1e-6.
Standard weights: a_j by j mod 7 = {0, ln 2, -3.5, -inf, 0, 1.25, -0.5} and one whole class at -inf, whose entries of `out`
must be the library's "absent class" value exactly.  Every forward runs on a workspace filled with 0xFF beforehand."""
import math

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import ws_poison

pytestmark = pytest.mark.gpu

NEG_INF = float("-inf")
LOG_EPS = math.log(1e-12)
LS0 = float(np.log(1 / 0.07))
KINDS = ("euclidean", "hypersphere_euclidean", "cosine", "dotproduct", "clip")
SHAPES = [(37, 4100, 96), (130, 1000, 64), (256, 2048, 512)]
ALL_TILES = 1920          # a multiple of every tile height
PATTERN = (0.0, math.log(2.0), -3.5, NEG_INF, 0.0, 1.25, -0.5)
DEAD_CLASS = 3
FWD, BWD = "nw_fwd_weighted_f32", "nw_bwd_query_weighted_f32"
SPIED = (FWD, BWD, "nw_fwd_window_f32", "nw_bwd_query_f32", "nw_fwd_f32", "nw_scores_f32", "nw_aggregate_f32")


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


def _spy(monkeypatch):
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


@pytest.fixture
def launches(monkeypatch):
    return _spy(monkeypatch)


@pytest.fixture(scope="module")
def absent(dev, ops):
    """What the library writes for a class that no row carries (logf(0 + 1e-12f) on the device): the plain head over a bank
    without class 1."""
    g = torch.Generator().manual_seed(3)
    s, q = torch.randn(64, 32, generator=g).to(dev), torch.randn(4, 32, generator=g).to(dev)
    sy = torch.zeros(64, dtype=torch.int64, device=dev)
    v = ops.nw_head(q, s, sy, 2, support_cache=ops.SplitBank(s, labels=sy))[0, 1].item()
    assert abs(v - LOG_EPS) < 4e-6
    return v


# ------------------------------------------------------------------------------------------------ data and reference
def _data(B, N, d, seed=None):
    g = torch.Generator().manual_seed(B * 7919 + N * 31 + d if seed is None else seed)
    return torch.randn(B, d, generator=g), torch.randn(N, d, generator=g)


def _sorted_labels(N, C=16):
    return (torch.arange(N) % C).sort().values


def _std_logw(sy, dead_class=DEAD_CLASS):
    a = torch.tensor(PATTERN, dtype=torch.float32)[torch.arange(len(sy)) % 7].clone()
    if dead_class is not None:
        a[sy == dead_class] = NEG_INF
    return a


def _class_windows(sy, B, C=16, seed=11):
    qy = torch.randint(0, C, (B,), generator=torch.Generator().manual_seed(seed))
    return torch.searchsorted(sy, qy), torch.searchsorted(sy, qy, right=True), qy


def _tensor_pair(pairs, B):
    return (torch.tensor([pairs[b % len(pairs)][0] for b in range(B)]), torch.tensor([pairs[b % len(pairs)][1] for b in range(B)]))


def _admitted(N, lo, hi, exclude):
    cols = torch.arange(N)
    inside = (cols >= lo.clamp(0, N)[:, None]) & (cols < hi.clamp(0, N)[:, None])
    return ~inside if exclude else inside


def _scores_f64(q, s, kind, ls=None, admit=None):
    """fp64 scores; with queries in an autograd graph the direct-difference form, where the distance of a pair that `admit`
    leaves out (a query's own copy in the bank) is not differentiated at 0."""
    grad = q.requires_grad
    q, s = q.double(), s.double()
    if kind in ("hypersphere_euclidean", "cosine", "clip"):
        q = q / q.norm(dim=-1, keepdim=True).clamp_min(1e-12)
        s = s / s.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    if kind in ("euclidean", "hypersphere_euclidean"):
        if not grad:
            return -torch.cdist(q, s, compute_mode="donot_use_mm_for_euclid_dist")
        d2 = (q[:, None, :] - s[None]).pow(2).sum(-1)
        if admit is not None:
            d2 = torch.where(admit, d2, torch.ones_like(d2))
        return -d2.sqrt()
    dot = q @ s.T
    if kind == "clip":
        return (ls.exp() if torch.is_tensor(ls) else math.exp(float(ls))) * dot
    return dot


def _head_f64(q, s, sy, C, a, window=None, exclude=False, kind="euclidean", ls=None):
    """-> (log-probs, lse, smax, number of dead queries), all from fp64 on the CPU."""
    N = s.shape[0]
    admit = (a > NEG_INF)[None].expand(q.shape[0], N)
    if window is not None:
        admit = admit & _admitted(N, window[0], window[1], exclude)
    sc = _scores_f64(q, s, kind, ls, admit) + torch.where(a > NEG_INF, a, torch.zeros_like(a)).double()[None]
    smax = sc.detach()[admit].abs().max().item() if bool(admit.any()) else 0.0
    sc = sc.masked_fill(~admit, NEG_INF)
    live = admit.any(dim=1, keepdim=True)
    w = torch.where(live, torch.softmax(torch.where(live, sc, torch.zeros_like(sc)), dim=-1), torch.zeros_like(sc))
    out = torch.log(w @ F.one_hot(sy, C).double() + 1e-12)
    lse = torch.where(live[:, 0], torch.logsumexp(torch.where(live, sc, torch.zeros_like(sc)), dim=-1),
                      torch.full_like(sc[:, 0], NEG_INF))
    return out, lse, smax, int((~live).sum())


def _close(got, ref, smax, what=""):
    got = got.detach().cpu().double()
    assert bool(torch.isfinite(got).all()), what
    err = (got - ref).abs().max().item()
    print(f"ERR {err:.3e} (atol {max(3e-5, 3e-6 * smax):.3e}, smax {smax:.1f}) {what}")
    np.testing.assert_allclose(got.numpy(), ref.detach().numpy(), rtol=1e-5, atol=max(3e-5, 3e-6 * smax), err_msg=what)


def _close_lse(got, ref, smax, what=""):
    got = got.detach().cpu().double()
    dead = ref == NEG_INF
    assert bool((got[dead] == NEG_INF).all()) and not bool(torch.isnan(got).any()), what
    np.testing.assert_allclose(got[~dead].numpy(), ref[~dead].numpy(), rtol=1e-5, atol=max(3e-5, 3e-6 * smax), err_msg=what)


def _poison(q, bank, N, C):
    need = ws_poison.fwd_workspace_bytes(q.shape[0], N, bank.shape[1], C)
    torch.cuda.synchronize()
    assert need > 0 and ws_poison.poison_cached_workspaces(need, q.device) >= need


def _fwd(ops, dev, q, s, sy, C, bank, a, window=None, exclude=False, kind="euclidean", ls=None):
    """(out, lse) of the weighted head on a poisoned workspace; q / s / sy on the device, a and the window from the CPU."""
    _poison(q, bank, s.shape[0], C)
    win = None if window is None else (window[0].to(dev), window[1].to(dev))
    return ops.nw_head_window(q, s, sy, C, bank, win, exclude, kind, ls, return_lse=True,
                              row_logw=None if a is None else a.to(dev))


class Bank:
    """Inputs on the CPU and the device, the class-sorted bank prepared once."""

    def __init__(self, ops, dev, B, N, d, C=16, seed=None, q=None, s=None, sy=None):
        self.q0, self.s0 = _data(B, N, d, seed)
        if q is not None:
            self.q0 = q
        if s is not None:
            self.s0 = s
        self.sy0 = _sorted_labels(N, C) if sy is None else sy
        self.q, self.s, self.sy = self.q0.to(dev), self.s0.to(dev), self.sy0.to(dev)
        self.bank = ops.SplitBank(self.s, labels=self.sy)
        self.B, self.N, self.d, self.C = B, N, d, C


_BANKS = {}


def _bank(ops, dev, B, N, d, C=16):
    if (B, N, d, C) not in _BANKS:
        _BANKS[(B, N, d, C)] = Bank(ops, dev, B, N, d, C)
    return _BANKS[(B, N, d, C)]


@pytest.fixture(scope="module", autouse=True)
def _drop_banks():
    yield
    _BANKS.clear()
    _GRAD_CASES.clear()


def _check(ops, dev, k, a, window=None, exclude=False, kind="euclidean", ls=None, absent=None, n_dead=None, what=""):
    out, lse = _fwd(ops, dev, k.q, k.s, k.sy, k.C, k.bank, a, window, exclude, kind, None if ls is None else torch.tensor(ls, device=dev))
    ref, ref_lse, smax, dead = _head_f64(k.q0, k.s0, k.sy0, k.C, a, window, exclude, kind, ls)
    assert out.shape == (k.B, k.C) and out.dtype == torch.float32
    _close(out, ref, smax, what)
    _close_lse(lse, ref_lse, smax, what + " lse")
    if n_dead is not None:
        assert dead == n_dead, (dead, n_dead)
    if absent is not None:
        assert bool((out[:, DEAD_CLASS] == absent).all()), "a class whose rows are all at -inf is an absent class, exactly"
    return out, lse


# ------------------------------------------------------------------------------------------------ 1. forward parity
@pytest.mark.parametrize("window", ["none", "kept", "excluded"])
@pytest.mark.parametrize("B,N,d", SHAPES)
def test_forward_parity(dev, ops, launches, absent, B, N, d, window):
    k = _bank(ops, dev, B, N, d)
    a = _std_logw(k.sy0)
    lo, hi, qy = _class_windows(k.sy0, B)
    win = None if window == "none" else (lo, hi)
    # a kept window of the class whose rows are all at -inf admits nothing that has a weight: those queries are dead
    n_dead = int((qy == DEAD_CLASS).sum()) if window == "kept" else 0
    _check(ops, dev, k, a, win, window == "excluded", absent=absent, n_dead=n_dead, what=f"{(B, N, d)} {window}")
    assert launches == [FWD], "fused at every shape the windowed head takes"


@pytest.mark.parametrize("kind", KINDS)
def test_score_kinds(dev, ops, launches, absent, kind):
    B, N, d = SHAPES[1]
    k = _bank(ops, dev, B, N, d)
    a = _std_logw(k.sy0)
    lo, hi, _ = _class_windows(k.sy0, B)
    ls = 2.5 if kind == "clip" else None
    for win, exclude in ((None, False), ((lo, hi), False), ((lo, hi), True)):
        _check(ops, dev, k, a, win, exclude, kind, ls, absent=absent, what=f"{kind} window={win is not None} exclude={exclude}")
    assert launches == [FWD] * 3


# ------------------------------------------------------------------------------------------------ 2. every tile height
@pytest.mark.parametrize("rs", [2, 4, 5, 6, 8, 10])
def test_every_tile_height(dev, ops, monkeypatch, absent, rs):
    from nwhead_amd import _lib
    monkeypatch.setenv("NW_TILE_RS", str(rs))
    _lib.sync_knobs()
    try:
        ops._WS_BYTES.clear()                      # sizes answered under another tile height
        BS = 16 * rs
        B, N, d = 70, BS * 3 + 20, 64              # the partial last tile included
        k = Bank(ops, dev, B, N, d)
        a = _std_logw(k.sy0)
        calls = _spy(monkeypatch)
        clo, chi, _ = _class_windows(k.sy0, B)
        pairs = [(BS, 2 * BS), (BS + 3, BS + 9), (BS - 1, BS + 1), (N - 30, N), (3 * BS, N), (0, BS), (5, 8), (BS, N),
                 (0, 1), (N - 1, N), (2 * BS, 2 * BS + 1), (2 * BS - 1, 2 * BS)]
        plo, phi = _tensor_pair(pairs, B)
        _check(ops, dev, k, a, absent=absent, what=f"rs={rs} no window")
        for exclude in (False, True):
            _check(ops, dev, k, a, (clo, chi), exclude, absent=absent, what=f"rs={rs} class windows exclude={exclude}")
            _check(ops, dev, k, a, (plo, phi), exclude, absent=absent, what=f"rs={rs} windows that cut tiles exclude={exclude}")
        assert calls == [FWD] * 5
        # zero weights: the windowed head's bits at this tile height (the hook adds nothing to the rounding of the scores)
        zero = torch.zeros(N)
        for kind in ("euclidean", "hypersphere_euclidean"):
            got = _fwd(ops, dev, k.q, k.s, k.sy, k.C, k.bank, zero, (plo, phi), True, kind)
            want = _fwd(ops, dev, k.q, k.s, k.sy, k.C, k.bank, None, (plo, phi), True, kind)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), kind
    finally:
        monkeypatch.delenv("NW_TILE_RS")
        _lib.sync_knobs()
        ops._WS_BYTES.clear()


# ------------------------------------------------------------------------------------------------ 3. bit identities
@pytest.mark.parametrize("kind", KINDS)
def test_zero_weights_are_the_windowed_head_bit_for_bit(dev, ops, kind):
    """(a) a == 0: the bits of nw_fwd_window_f32 with the same window; without a window, of the kept window [0, N)."""
    k = _bank(ops, dev, *SHAPES[0])
    ls = torch.tensor(2.5, device=dev) if kind == "clip" else None
    zero = torch.zeros(k.N)
    lo, hi, _ = _class_windows(k.sy0, k.B)
    plo, phi = _tensor_pair([(ALL_TILES + 5, ALL_TILES + 20), (ALL_TILES, 2 * ALL_TILES), (4000, k.N), (ALL_TILES - 1, ALL_TILES + 1)], k.B)
    whole = (torch.zeros(k.B, dtype=torch.int64), torch.full((k.B,), k.N))
    for win, exclude in (((lo, hi), False), ((lo, hi), True), ((plo, phi), False), ((plo, phi), True)):
        got = _fwd(ops, dev, k.q, k.s, k.sy, k.C, k.bank, zero, win, exclude, kind, ls)
        want = _fwd(ops, dev, k.q, k.s, k.sy, k.C, k.bank, None, win, exclude, kind, ls)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    got = _fwd(ops, dev, k.q, k.s, k.sy, k.C, k.bank, zero, None, False, kind, ls)
    want = _fwd(ops, dev, k.q, k.s, k.sy, k.C, k.bank, None, whole, False, kind, ls)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


@pytest.mark.parametrize("lo,hi", [(ALL_TILES + 5, ALL_TILES + 20), (ALL_TILES, 2 * ALL_TILES), (ALL_TILES - 1, ALL_TILES + 1),
                                   (4000, 4100), (4097, 4100), (0, ALL_TILES), (0, 1), (700, 2900)])
def test_minus_inf_rows_are_an_excluded_window_bit_for_bit(dev, ops, lo, hi):
    """(b) a = -inf on rows [lo, hi), 0 elsewhere, no window: the bits of the excluded window [lo, hi), out and lse, with the
    edges inside tiles and on the boundaries of every tile height."""
    k = _bank(ops, dev, *SHAPES[0])
    a = torch.zeros(k.N)
    a[lo:hi] = NEG_INF
    win = (torch.full((k.B,), lo), torch.full((k.B,), hi))
    got, want = _fwd(ops, dev, k.q, k.s, k.sy, k.C, k.bank, a), _fwd(ops, dev, k.q, k.s, k.sy, k.C, k.bank, None, win, True)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_two_calls_give_the_same_bits(dev, ops):
    """(c) on a poisoned workspace each."""
    k = _bank(ops, dev, *SHAPES[0])
    a = _std_logw(k.sy0)
    lo, hi, _ = _class_windows(k.sy0, k.B)
    for win, exclude in ((None, False), ((lo, hi), True)):
        one, two = _fwd(ops, dev, k.q, k.s, k.sy, k.C, k.bank, a, win, exclude), _fwd(ops, dev, k.q, k.s, k.sy, k.C, k.bank, a, win, exclude)
        assert bool(torch.isfinite(one[0]).all()) and torch.equal(one[0], two[0]) and torch.equal(one[1], two[1])


# ------------------------------------------------------------------------------------------------ 4. order of operations
def test_weight_is_added_before_the_tile_maximum(dev, ops, launches):
    """a = +100 on one far row in each of three tiles, a = -100 on every query's exact copy in the bank (distance 0).  A tile
    maximum taken before the weight is 0 (the copy) and the far row's exponential 2^((100 - D) log2 e) overflows."""
    B, N, d, C = 64, 1000, 64, 16
    q0, s0 = _data(B, N, d, seed=77)
    rows = torch.arange(B) * 15 + 7                  # the queries' copies, spread over the tiles
    q0 = s0[rows].clone()
    k = Bank(ops, dev, B, N, d, C, q=q0, s=s0)
    a = torch.zeros(N)
    a[rows] = -100.0
    far = torch.tensor([10, 500, 990])               # three tiles at every tile height (<= 160 rows), none a query's copy
    assert not bool(torch.isin(far, rows).any())
    assert (q0[:, None, :] - s0[far][None]).norm(dim=-1).min().item() > 5.0
    a[far] = 100.0
    out, lse = _check(ops, dev, k, a, what="+100 / -100")
    assert bool(torch.isfinite(lse).all()) and launches == [FWD]


# ------------------------------------------------------------------------------------------------ 5. dead queries and tiles
def test_dead_queries_by_weight(dev, ops, launches, absent):
    B, N, d = 70, 1000, 64
    k = _bank(ops, dev, B, N, d)
    a = _std_logw(k.sy0, dead_class=None)
    a[255:300] = NEG_INF                             # (inside one class: no class window is left without a row)
    # a window that admits only -inf rows, for a whole 16-query wave (queries 16..31) and three strays beside live ones
    lo, hi, _ = _class_windows(k.sy0, B)
    dead_q = list(range(16, 32)) + [0, 40, 69]
    lo[dead_q], hi[dead_q] = 260, 290
    out, lse = _check(ops, dev, k, a, (lo, hi), False, n_dead=len(dead_q), what="windows of -inf rows")
    assert bool((out[dead_q] == absent).all()) and bool((lse[dead_q] == NEG_INF).all())
    # every weight at -inf: every query is dead, through the wave-wide early exit of every tile
    out, lse = _check(ops, dev, k, torch.full((N,), NEG_INF), n_dead=B, what="all -inf")
    assert bool((out == absent).all()) and bool((lse == NEG_INF).all())
    out, lse = _check(ops, dev, k, torch.full((N,), NEG_INF), (lo, hi), True, n_dead=B, what="all -inf, excluded windows")
    assert bool((out == absent).all()) and launches == [FWD] * 3


@pytest.mark.parametrize("rs", [4, 8])
def test_dead_tile_between_live_tiles(dev, ops, monkeypatch, rs):
    from nwhead_amd import _lib
    monkeypatch.setenv("NW_TILE_RS", str(rs))
    _lib.sync_knobs()
    try:
        ops._WS_BYTES.clear()
        BS = 16 * rs
        k = Bank(ops, dev, 70, 3 * BS + 20, 64)
        a = _std_logw(k.sy0, dead_class=None)
        a[BS:2 * BS] = NEG_INF                       # the whole second tile: dead for every query, live tiles either side
        _check(ops, dev, k, a, n_dead=0, what=f"rs={rs} dead tile")
        lo, hi = torch.full((70,), BS), torch.full((70,), 2 * BS + 5)
        lo[::3], hi[::3] = BS + 1, 2 * BS            # every third query sees nothing but the dead tile
        _check(ops, dev, k, a, (lo, hi), False, n_dead=len(range(0, 70, 3)), what=f"rs={rs} dead tile, kept windows")
    finally:
        monkeypatch.delenv("NW_TILE_RS")
        _lib.sync_knobs()
        ops._WS_BYTES.clear()


# ------------------------------------------------------------------------------------------------ 6. meaning
def test_weight_ln2_is_the_row_twice(dev, ops):
    """Weight ln 2 on row j = the bank with row j duplicated (next to itself: still class-sorted) and rebuilt."""
    B, N, d, C = 37, 1000, 64, 16
    q0, s0 = _data(B, N, d, seed=5)
    sy0 = _sorted_labels(N, C)
    js = [3, 511, 998]
    for i, j in enumerate(js):                       # queries near the rows, so that their weight matters
        q0[4 * i:4 * i + 4] = s0[j] + 0.5 * q0[4 * i:4 * i + 4]
    k = Bank(ops, dev, B, N, d, C, q=q0, s=s0)
    a = torch.zeros(N)
    a[js] = math.log(2.0)
    out, _ = _fwd(ops, dev, k.q, k.s, k.sy, C, k.bank, a)
    idx = torch.tensor(sorted(list(range(N)) + js))
    s2, sy2 = s0[idx].to(dev), sy0[idx].to(dev)
    twice = ops.nw_head(k.q, s2, sy2, C, support_cache=ops.SplitBank(s2, labels=sy2))
    plain = ops.nw_head(k.q, k.s, k.sy, C, support_cache=k.bank)
    smax = _head_f64(q0, s0, sy0, C, a)[2]
    _close(out, twice.cpu().double(), smax, "ln 2 vs the row twice")
    assert (out - plain).abs().max().item() > 1e-2, "the weights matter in this case"


# ------------------------------------------------------------------------------------------------ 7. backward
GRAD_SHAPES = [(64, 1024, 64, 5), (129, 257, 160, 1000), (33, 4099, 64, 7)]
_GRAD_CASES = {}


class GradCase:
    def __init__(self, ops, dev, B, N, d, C, kind):
        g = torch.Generator().manual_seed(B + N + d + C)
        q0, s0 = torch.randn(B, d, generator=g), torch.randn(N, d, generator=g)
        if kind == "dotproduct":
            q0, s0 = q0 * d ** -0.25, s0 * d ** -0.25
        sy0 = torch.randint(0, C, (N,), generator=g).sort().values
        self.k = Bank(ops, dev, B, N, d, C, q=q0, s=s0, sy=sy0)
        self.kind, self.shape = kind, (B, N, d, C)
        self.gout = torch.randn(B, C, generator=torch.Generator().manual_seed(7))
        self.a = _std_logw(sy0, dead_class=int(sy0[N // 2]))
        self.memo = {}

    def ls(self, dev=None, grad=True):
        if self.kind != "clip":
            return None
        return torch.tensor(LS0, dtype=torch.float64 if dev is None else torch.float32, device=dev, requires_grad=grad)

    def ref(self, tag, a, window=None, exclude=False, q0=None):
        if tag not in self.memo:
            k = self.k
            q = (k.q0 if q0 is None else q0).double().requires_grad_(True)
            ls = self.ls()
            out, _, _, dead = _head_f64(q, k.s0, k.sy0, k.C, a, window, exclude, self.kind, ls)
            ins = (q,) + ((ls,) if ls is not None else ())
            gr = torch.autograd.grad((out * self.gout.double()).sum(), ins)
            self.memo[tag] = (gr[0], gr[1] if ls is not None else None, dead)
        return self.memo[tag]


def _grad_case(ops, dev, shape, kind):
    if (shape, kind) not in _GRAD_CASES:
        _GRAD_CASES[(shape, kind)] = GradCase(ops, dev, *shape, kind)
    return _GRAD_CASES[(shape, kind)]


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


def _direct(ops, dev, c, a, window=None, exclude=False, row_chunks=0, q0=None, weighted=True, poison=0xFF):
    """The forward through ops, then nw_bwd_query_weighted_f32 (or, ``weighted=False``, nw_bwd_query_f32) called directly
    on a poisoned workspace of the caller's -> (gq, glogit_scale)."""
    from nwhead_amd import _lib
    lib = _lib.load()
    k = c.k
    B, N, d, C = c.shape
    kid = ops.SCORE_KINDS[c.kind]
    q = k.q if q0 is None else q0.to(dev)
    ls = c.ls(dev, False)
    win = None if window is None else tuple(t.to(dev).to(torch.int32).contiguous() for t in window)
    ad = None if a is None else a.to(dev)
    with torch.no_grad():
        if weighted or win is not None:
            out, lse = ops.nw_head_window(q, k.s, k.sy, C, k.bank, win, exclude, c.kind, ls, return_lse=True, row_logw=ad if weighted else None)
        else:
            whole = (torch.zeros(B, dtype=torch.int32, device=dev), torch.full((B,), N, dtype=torch.int32, device=dev))
            out, lse = ops.nw_head_window(q, k.s, k.sy, C, k.bank, whole, False, c.kind, ls, return_lse=True)
    need = lib.nw_bwd_query_workspace_bytes(B, N, d, C, row_chunks)
    assert need > 0
    ws = torch.full((need,), poison, dtype=torch.uint8, device=dev)
    gq, gls, g = torch.empty(B, d, device=dev), torch.empty((), device=dev), c.gout.to(dev).contiguous()
    lo, hi = (None, None) if win is None else (win[0].data_ptr(), win[1].data_ptr())
    bank = (k.bank.split.data_ptr(), k.bank.scale.data_ptr(), k.bank.norm2.data_ptr(), k.sy.data_ptr())
    tail = (lse.data_ptr(), out.data_ptr(), g.data_ptr(), gq.data_ptr(), gls.data_ptr(), ws.data_ptr(), need, B, N, d, C, kid,
            None if ls is None else ls.data_ptr(), row_chunks, None)
    if weighted:
        _lib.check(lib.nw_bwd_query_weighted_f32(q.data_ptr(), *bank, ad.data_ptr(), lo, hi, int(exclude), *tail), BWD)
    else:
        _lib.check(lib.nw_bwd_query_f32(q.data_ptr(), *bank, lo, hi, int(exclude), *tail), "nw_bwd_query_f32")
    torch.cuda.synchronize()
    return gq, gls


def _loo(c):
    """Queries that are bank rows, each without itself; -1 (no row left out) for every fourth."""
    B, N = c.shape[:2]
    rows = (torch.arange(B) * (N // B)) + 1
    q0 = c.k.s0[rows].clone()
    lo = rows.clone()
    hi = rows + 1
    hi[::4] = lo[::4]
    return q0, (lo, hi)


@pytest.mark.parametrize("kind", ("euclidean", "cosine"))
@pytest.mark.parametrize("shape", GRAD_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_backward_parity(ops, dev, launches, shape, kind):
    c = _grad_case(ops, dev, shape, kind)
    k = c.k
    q = k.q.clone().requires_grad_(True)
    out = ops.nw_head_bank(q, k.s, k.sy, k.C, k.bank, kind, row_logw=c.a.to(dev))
    out.backward(c.gout.to(dev))
    rq, _, dead = c.ref("std", c.a)
    assert dead == 0 and launches == [FWD, BWD]
    _gclose(q.grad, rq, f"gq {kind} {shape}")
    for rc in (0, 3):
        gq, _ = _direct(ops, dev, c, c.a, row_chunks=rc)
        _gclose(gq, rq, f"gq {kind} {shape} row_chunks={rc}")
        if rc == 0:
            assert torch.equal(gq, q.grad)
    # leave-one-out of the bank's own rows
    q0, win = _loo(c)
    rq, _, dead = c.ref("loo", c.a, win, True, q0)
    for rc in (0, 3):
        gq, _ = _direct(ops, dev, c, c.a, win, True, rc, q0)
        _gclose(gq, rq, f"gq leave-one-out {kind} {shape} row_chunks={rc}")
    # through autograd as well
    q = q0.to(dev).requires_grad_(True)
    ops.nw_head_bank(q, k.s, k.sy, k.C, k.bank, kind, row_window=(win[0].to(dev), win[1].to(dev)), exclude=True,
                     row_logw=c.a.to(dev)).backward(c.gout.to(dev))
    _gclose(q.grad, rq, f"gq leave-one-out {kind} {shape} autograd")


def test_backward_clip_logit_scale(ops, dev, launches):
    c = _grad_case(ops, dev, GRAD_SHAPES[0], "clip")
    k = c.k
    q, ls = k.q.clone().requires_grad_(True), c.ls(dev)
    ops.nw_head_bank(q, k.s, k.sy, k.C, k.bank, "clip", ls, row_logw=c.a.to(dev)).backward(c.gout.to(dev))
    rq, rls, _ = c.ref("std", c.a)
    _gclose(q.grad, rq, "gq clip")
    _gclose(ls.grad, rls, "logit_scale.grad clip", ls=True)
    for rc in (0, 3):
        gq, gls = _direct(ops, dev, c, c.a, row_chunks=rc)
        _gclose(gq, rq, f"gq clip row_chunks={rc}")
        _gclose(gls, rls, f"logit_scale.grad clip row_chunks={rc}", ls=True)
    assert launches[:2] == [FWD, BWD]


@pytest.mark.parametrize("kind", ("euclidean", "cosine"))
def test_backward_bit_identities(ops, dev, kind):
    """(a) a == 0: nw_bwd_query_f32's bits with the same window (none: the head of the kept window [0, N) forward, no window
    backward).  (b) a = -inf on [lo, hi): the bits of the excluded window [lo, hi)."""
    shape = GRAD_SHAPES[2]
    c = _grad_case(ops, dev, shape, kind)
    B, N = shape[:2]
    zero = torch.zeros(N)
    q0, win = _loo(c)
    for rc in (0, 3):
        assert torch.equal(_direct(ops, dev, c, zero, row_chunks=rc)[0], _direct(ops, dev, c, None, row_chunks=rc, weighted=False)[0])
        assert torch.equal(_direct(ops, dev, c, zero, win, True, rc, q0)[0], _direct(ops, dev, c, None, win, True, rc, q0, weighted=False)[0])
    for lo, hi in ((100, 1000), (64, 128), (4090, N), (63, 65)):      # 64-row tiles of the backward: inside and on boundaries
        a = zero.clone()
        a[lo:hi] = NEG_INF
        w = (torch.full((B,), lo), torch.full((B,), hi))
        assert torch.equal(_direct(ops, dev, c, a)[0], _direct(ops, dev, c, None, w, True, weighted=False)[0]), (lo, hi)


def test_backward_dead_queries_get_zero_rows(ops, dev):
    shape = GRAD_SHAPES[2]
    c = _grad_case(ops, dev, shape, "euclidean")
    B, N = shape[:2]
    a = c.a.clone()
    a[1000:2000] = NEG_INF
    lo, hi = torch.zeros(B, dtype=torch.int64), torch.full((B,), N)
    dead_q = [0, 5, 16, 17, 32]
    lo[dead_q], hi[dead_q] = 1200, 1300               # a kept window of -inf rows
    rq, _, dead = c.ref("dead", a, (lo, hi), False)
    assert dead == len(dead_q)
    for rc in (0, 3):
        gq, _ = _direct(ops, dev, c, a, (lo, hi), False, rc)
        _gclose(gq, rq, f"gq with dead queries row_chunks={rc}")
        assert bool((gq[dead_q] == 0).all())
    gq, _ = _direct(ops, dev, c, torch.full((N,), NEG_INF))
    assert bool((gq == 0).all())


def _trap_case():
    """A large positive weight on a NEAR row (CPU only): (q0, s0, sy0, a, gout, true gq, gq of the wrong formula)."""
    B, N, d, C = GRAD_SHAPES[0]
    g = torch.Generator().manual_seed(123)
    s0 = torch.randn(N, d, generator=g)
    sy0 = torch.randint(0, C, (N,), generator=g).sort().values
    rows = torch.arange(B) * 16 + 3
    q0 = s0[rows] + 0.05 * torch.randn(B, d, generator=g)          # distance ~0.4 to the near row, ~11 to the others
    a = torch.zeros(N)
    a[rows] = 3.0
    gout = torch.randn(B, C, generator=torch.Generator().manual_seed(7))
    q, s = q0.double(), s0.double()
    sc = (-(q[:, None, :] - s[None]).pow(2).sum(-1).sqrt()).requires_grad_(True)
    w = torch.softmax(sc + a.double()[None], dim=-1)
    out = torch.log(w @ F.one_hot(sy0, C).double() + 1e-12)
    dS, = torch.autograd.grad((out * gout.double()).sum(), sc)
    diff = s[None] - q[:, None, :]                                   # d score / d q = (s - q) / D
    D = -sc.detach()
    true = (dS / D)[..., None].mul(diff).sum(1)
    wrong = (dS / (D - a.double()[None]))[..., None].mul(diff).sum(1)   # the distance taken from the WEIGHTED score
    return q0, s0, sy0, a, gout, true, wrong


def test_distance_derivative_takes_the_raw_score(ops, dev):
    """A weight of +3 on a row at distance ~0.4: d score / d q = (s - q) / D must use D = -score, not -(score + a) = D - 3.
    Confirmed on the CPU in fp64 first: the wrong formula misses the bar (1e-4 of max |gq|) by a normalised error of 1.04
    -- four orders of magnitude -- so a kernel that hands bwd_pair_coeff the weighted score cannot pass here."""
    q0, s0, sy0, a, gout, true, wrong = _trap_case()
    scale = max(true.abs().max().item(), 1e-3)
    margin = (wrong - true).abs().max().item() / scale
    print(f"TRAP wrong-formula normalised error {margin:.3e}")
    assert margin > 1e-2
    B, N, d, C = GRAD_SHAPES[0]
    k = Bank(ops, dev, B, N, d, C, q=q0, s=s0, sy=sy0)
    q = k.q.clone().requires_grad_(True)
    ops.nw_head_bank(q, k.s, k.sy, C, k.bank, row_logw=a.to(dev)).backward(gout.to(dev))
    qr = q0.double().requires_grad_(True)
    ref, = torch.autograd.grad((_head_f64(qr, s0, sy0, C, a)[0] * gout.double()).sum(), qr)
    assert (ref - true).abs().max().item() / scale < 1e-9
    _gclose(q.grad, ref, "gq with +3 on a near row")


# ------------------------------------------------------------------------------------------------ 8. Python surface
def test_nw_head_equals_nw_head_bank_forward(ops, dev, launches):
    k = _bank(ops, dev, *SHAPES[1])
    a = _std_logw(k.sy0).to(dev)
    lo, hi, _ = _class_windows(k.sy0, k.B)
    win = (lo.to(dev), hi.to(dev))
    with torch.no_grad():
        h1 = ops.nw_head(k.q, k.s, k.sy, k.C, support_cache=k.bank, row_logw=a)
        h2 = ops.nw_head(k.q, k.s, k.sy, k.C, support_cache=k.bank, row_logw=a, row_window=win, exclude=True)
    q = k.q.clone().requires_grad_(True)
    b1 = ops.nw_head_bank(q, k.s, k.sy, k.C, k.bank, row_logw=a)
    b2 = ops.nw_head_bank(q, k.s, k.sy, k.C, k.bank, row_logw=a, row_window=win, exclude=True)
    assert b1.requires_grad and torch.equal(h1, b1.detach()) and torch.equal(h2, b2.detach())
    assert launches == [FWD] * 4
    with pytest.raises(ValueError):
        ops.nw_head(q, k.s, k.sy, k.C, support_cache=k.bank, row_logw=a)          # gradients: nw_head_bank's
    with pytest.raises(ValueError):
        ops.nw_head(k.q, k.s, k.sy, k.C, support_cache=k.bank, row_logw=a[:-1])
    # None leaves the calls what they were
    with torch.no_grad():
        assert torch.equal(ops.nw_head(k.q, k.s, k.sy, k.C, support_cache=k.bank, row_logw=None), ops.nw_head(k.q, k.s, k.sy, k.C, support_cache=k.bank))


@pytest.mark.parametrize("case", ["fp16 bank", "unsorted labels", "N = 20"])
def test_fallback_route_agrees(ops, dev, launches, case):
    B, d, C = 33, 64, 16
    N = 20 if case == "N = 20" else 1000
    q0, s0 = _data(B, N, d, seed=9)
    sy0 = _sorted_labels(N, C)
    if case == "unsorted labels":
        sy0 = sy0[torch.randperm(N, generator=torch.Generator().manual_seed(2))]
    q, s, sy = q0.to(dev), s0.to(dev), sy0.to(dev)
    bank = ops.SplitBank(s, labels=sy, precision="fp16") if case == "fp16 bank" else ops.SplitBank(s, labels=sy)
    a = _std_logw(sy0)
    lo = torch.arange(B) % N
    hi = lo + 1 + N // 2
    lo[5], hi[5] = 3, 3                               # an empty window; the standard pattern leaves nobody else dead
    for win, exclude in ((None, False), ((lo, hi), False), ((lo, hi), True)):
        del launches[:]
        out, lse = _fwd(ops, dev, q, s, sy, C, bank, a, win, exclude)
        assert FWD not in launches and "nw_aggregate_f32" in launches, launches
        ref, ref_lse, smax, dead = _head_f64(q0, s0, sy0, C, a, win, exclude)
        assert dead == (1 if win is not None and not exclude else 0)
        _close(out, ref, smax, f"{case} matrix route")
        _close_lse(lse, ref_lse, smax, f"{case} matrix route lse")
        if case == "unsorted labels":                 # the fused route over the same rows, class-sorted
            order = torch.argsort(sy0, stable=True)
            if win is None:
                s2, sy2 = s0[order].to(dev), sy0[order].to(dev)
                del launches[:]
                fused, _ = _fwd(ops, dev, q, s2, sy2, C, ops.SplitBank(s2, labels=sy2), a[order])
                assert launches == [FWD]
                _close(fused, out.cpu().double(), smax, "fused vs matrix route")
    qg = q.clone().requires_grad_(True)
    with pytest.raises(ops.NWHipError):                # no gradient route that knows the weights here
        ops.nw_head_bank(qg, s, sy, C, bank, row_logw=a.to(dev))


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


def test_nwnet_round_trip(ops, dev, launches):
    C, n = 6, 40
    net, g, din = _toy_net(dev, [n] * C)
    N = net.full_feat.shape[0]
    assert N == C * n and net.support_weights is None
    B = 24
    x = torch.randn(B, din, generator=g).to(dev)
    sy0 = net.full_y.cpu()
    a = _std_logw(sy0, dead_class=2)
    with torch.no_grad():
        plain = net.predict(x, 'full')
    with pytest.raises(ValueError):
        net.set_support_weights(torch.full((N,), float("nan")))
    with pytest.raises(ValueError):
        net.set_support_weights(torch.full((N,), float("inf")))
    with pytest.raises(ValueError):
        net.set_support_weights(torch.zeros(N - 1))
    assert net.support_weights is None
    net.set_support_weights(a)
    del launches[:]

    def ref(qfeat, window=None):
        return _head_f64(qfeat.cpu(), net.full_feat.cpu(), sy0, C, a, window, window is not None)

    with torch.no_grad():
        qfeat = net.featurizer(x)
        out = net.predict(x, 'full')
        r, _, smax, _ = ref(qfeat)
        _close(out, r, smax, "predict('full')")
        assert not torch.equal(out, plain) and bool((out[:, 2] < LOG_EPS + 1e-3).all())
        rows = torch.randint(0, N, (B,), generator=g)
        rows[::4] = -1
        lo = rows.clamp(min=0)
        win = (lo, torch.where(rows < 0, lo, lo + 1))
        out = net.predict(x, 'full', leave_out=rows.to(dev))
        _close(out, ref(qfeat, win)[0], smax, "predict('full', leave_out)")
        loo = net.predict_loo(batch_size=100)
        every = torch.arange(N)
        r = _head_f64(net.full_feat.cpu(), net.full_feat.cpu(), sy0, C, a, (every, every + 1), True)
        _close(loo, r[0], r[2], "predict_loo")
    assert launches and set(launches) == {FWD}
    # forward_bank: the weighted head, differentiable in the featurizer
    del launches[:]
    gout = torch.randn(B, C, generator=g)
    net.zero_grad()
    out = net.forward_bank(x, leave_out=rows.to(dev))
    out.backward(gout.to(dev))
    assert launches == [FWD, BWD]
    feat64 = nn.Linear(din, net.full_feat.shape[1]).double()
    feat64.load_state_dict({k_: v.detach().cpu().double() for k_, v in net.featurizer.state_dict().items()})
    o64 = _head_f64(feat64(x.cpu().double()), net.full_feat.cpu(), sy0, C, a, win, True)[0]
    (o64 * gout.double()).sum().backward()
    _gclose(net.featurizer.weight.grad, feat64.weight.grad, "featurizer.weight.grad through forward_bank")
    # the weights survive a refresh (rows keep their identity) ...
    feat_before = net.full_feat.cpu().clone()
    net.refresh_bank(rows.to(dev))
    assert net.support_weights is not None and torch.equal(net.support_weights.cpu(), a)
    with torch.no_grad():     # (fresh queries: those of the refresh now have exact copies in the bank, at a distance that the
        #                        matmul form of the kernels does not resolve to the bound)
        x2 = torch.randn(B, din, generator=g).to(dev)
        r2, _, smax2, _ = _head_f64(net.featurizer(x2).cpu(), net.full_feat.cpu(), sy0, C, a)
        _close(net.predict(x2, 'full'), r2, smax2, "predict('full') after refresh_bank")
        before = _head_f64(net.featurizer(x2).cpu(), feat_before, sy0, C, a)[0]
        assert (before - r2).abs().max().item() > 1e-3, "the refreshed rows are what is read"
    # ... are cleared by None and by precompute()
    net.set_support_weights(None)
    assert net.support_weights is None
    net.set_support_weights(a)
    net.precompute()
    assert net.support_weights is None
    with torch.no_grad():
        del launches[:]
        net.predict(x, 'full')
    assert FWD not in launches


def test_nwnet_balance_full_weights(ops, dev):
    counts = [40, 7, 25, 3]
    net, g, din = _toy_net(dev, counts, balance_full="weights")
    assert net.full_y.cpu().tolist() == [c for c, n in enumerate(counts) for _ in range(n)]
    w = net.support_weights
    assert w is not None and torch.equal(w, ops.class_balance_logw(net.full_y, len(counts)))
    mass = torch.zeros(len(counts), dtype=torch.float64).index_add_(0, net.full_y.cpu(), w.cpu().double().exp())
    np.testing.assert_allclose(mass.numpy(), 1.0 / len(counts), rtol=1e-5)
    x = torch.randn(16, din, generator=g).to(dev)
    with torch.no_grad():
        out = net.predict(x, 'full')
        r, _, smax, _ = _head_f64(net.featurizer(x).cpu(), net.full_feat.cpu(), net.full_y.cpu(), len(counts), w.cpu())
    _close(out, r, smax, "balance_full='weights'")
    base, _, _ = _toy_net(dev, counts)
    assert base.support_weights is None and base.full_feat.shape[0] == min(counts) * len(counts)


def test_write_between_forward_and_backward_is_refused(ops, dev):
    k = _bank(ops, dev, *SHAPES[1])
    a = _std_logw(k.sy0).to(dev)
    q = k.q.clone().requires_grad_(True)
    out = ops.nw_head_bank(q, k.s, k.sy, k.C, k.bank, row_logw=a)
    a[5] = 0.25
    with pytest.raises(RuntimeError, match="row_logw"):
        out.sum().backward()
    a64 = _std_logw(k.sy0).double().to(dev)              # a converted copy is read: the caller's tensor is still watched
    out = ops.nw_head_bank(q, k.s, k.sy, k.C, k.bank, row_logw=a64)
    a64.mul_(2)
    with pytest.raises(RuntimeError, match="row_logw"):
        out.sum().backward()
    out = ops.nw_head_bank(q, k.s, k.sy, k.C, k.bank, row_logw=a)
    out.sum().backward()
    assert bool(torch.isfinite(q.grad).all())


def test_no_score_matrix_is_allocated(ops, dev):
    B, N, d, C = 64, 65536, 64, 7
    g = torch.Generator().manual_seed(1)
    s = torch.randn(N, d, generator=g).to(dev)
    sy0 = (torch.arange(N) % C).sort().values
    sy = sy0.to(dev)
    q0 = torch.randn(B, d, generator=g).to(dev)
    t = torch.randint(0, C, (B,), generator=g).to(dev)
    a = _std_logw(sy0, dead_class=None).to(dev)
    bank = ops.SplitBank(s, labels=sy)
    matrix = B * N * 4
    # the forward's scratch is the process-wide buffer of every inference call of this shape: warmed, like the bank
    ops._WS_CACHE.clear()
    with torch.no_grad():
        ops.nw_head(q0, s, sy, C, support_cache=bank, row_logw=a)
    q = q0.clone().requires_grad_(True)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.memory_allocated(dev)
    F.nll_loss(ops.nw_head_bank(q, s, sy, C, bank, row_logw=a), t).backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(dev) - before
    print(f"MEM weighted nw_head_bank {peak} bytes, one score matrix {matrix} bytes")
    assert peak < matrix and bool(torch.isfinite(q.grad).all())
