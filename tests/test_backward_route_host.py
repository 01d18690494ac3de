"""Which of its three product routes the head's backward takes, and how much workspace it asks for, on the host: no GPU.

The expected values are NOT read back from the library: `Rule` below restates DESIGN.md 4.6a (the route rule, the K-splits
and the areas each route needs), and the library's plan (plan_bwd in backward.hip, through nw_debug_bwd_plan,
nw_bwd_workspace_bytes and nw_bwd_uses_split) is held to it: route, row stride, chunk counts, every area's size, the total.
The map itself is checked like the forward's (tests/test_fwd_workspace_host.py), and the totals and split answers on a grid
around every threshold are those of the library before the plan existed (tests/golden/bwd_workspace_bytes.npz).
  VALU    everything else
  fp32 matrix cores   shared supports, d % 4 == 0, B N d >= 2^22, unless bwd_no_mfma = 1
  split fp16          the above and d % 32 == 0 and (80 + ld + C) floats <= 150 KiB with ld = N rounded up to 32
                      and, unless bwd_split = 1, B >= 16 and N >= 256; never with bwd_split = 0
"""
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NW_OK, NW_ERR_INVALID_ARG, NW_ERR_UNSUPPORTED = 0, -1, -2
UNSET = -2 ** 31
LDS_LAUNCH_BYTES = 160 * 1024                # past it the launcher refuses
LDS_SPLIT_FLOATS = 150 * 1024 // 4          # 38400: the coefficient kernel's LDS on the split route (80 + ld + C floats)
XGEMM_TAIL = 512 // 4                        # floats readable past the last row of every split-row operand


@pytest.fixture(scope="module")
def L():
    from nwhead_amd import _lib
    _lib.load()
    return _lib


@pytest.fixture
def knobs(L):
    """Set bwd_split / bwd_no_mfma for one test; afterwards they are what sync_knobs() last forwarded."""
    lib = L.load()

    def set_(**kw):
        for k, v in kw.items():
            assert lib.nw_debug_set(k.encode(), UNSET if v is None else v) == 0
    set_(bwd_split=None, bwd_no_mfma=None, xgemm_wgs=None)
    yield set_
    for k in ("bwd_split", "bwd_no_mfma", "xgemm_wgs"):
        lib.nw_debug_set(k.encode(), L._knob_state.get(k, UNSET))


def up(x, m):
    return (x + m - 1) // m * m


class Rule:
    """DESIGN.md 4.6a, restated."""

    def __init__(self, split_knob=None, no_mfma=False, xgemm_wgs=None):
        self.split_knob, self.no_mfma, self.xgemm_wgs = split_knob, no_mfma, xgemm_wgs

    def mfma(self, B, N, d, sup=0):
        return (not self.no_mfma) and not sup and d % 4 == 0 and B * N * d >= 2 ** 22

    def split(self, B, N, d, C, sup=0):
        if self.split_knob == 0 or not self.mfma(B, N, d, sup) or d % 32:
            return False
        if 80 + up(N, 32) + C > LDS_SPLIT_FLOATS:
            return False
        return True if self.split_knob == 1 else (B >= 16 and N >= 256)

    def route(self, B, N, d, C, sup=0):
        return "split" if self.split(B, N, d, C, sup) else "mfma" if self.mfma(B, N, d, sup) else "valu"

    @staticmethod
    def _chunks(M, Nn, K, tm, tn, tk, target, min_k):
        tiles = -(-M // tm) * -(-Nn // tn)
        want = 1 if tiles >= target else -(-target // tiles)
        want = min(want, max(K // min_k, 1))
        kc = up(-(-K // want), tk)
        return -(-K // kc)

    def plan(self, B, N, d, C, sup=0):
        """(route, ld, cq, cs, the fifteen area sizes in the order of _lib.BWD_AREAS, total): every area a whole number of
        256-byte units, empty where the route does not use it."""
        route = self.route(B, N, d, C, sup)
        split, cores = route == "split", route != "valu"
        ld = up(N, 32) if split else up(N, 4) if cores else N
        cq = cs = 0
        if split:
            wgs = self.xgemm_wgs if (self.xgemm_wgs or 0) > 0 else 256
            cq = self._chunks(B, d, N, 128, 64, 32, wgs, 128)                 # first product: M = B, K = N
            cs = self._chunks(N, d, B, 128, 64, 32, wgs, 128)                 # second product: M = N, K = B
        elif cores:
            cq = self._chunks(B, d, N, 128, 128, 16, 512, 64)
            cs = self._chunks(N, d, B, 128, 128, 16, 512, 64)
        nq, ns = (cq * B * d if cq > 1 else 0), (cs * N * d if cs > 1 else 0)
        floats = [B * ld + (XGEMM_TAIL if split else 0), B * ld, B, B, B, B * N if sup else N,          # A Rs rq gls qn2 sn2
                  N if cores else 0,                                                                     # rs
                  N * d + XGEMM_TAIL if split else 0, N if split else 0,                                 # s_split s_scale
                  up(B, 32) * d + XGEMM_TAIL if split else 0, B if split else 0, B if split else 0,      # q_split ascale qv
                  1 if split else 0,                                                                     # gfac
                  nq if split else max(nq, ns), ns if split else 0]                                      # part part2
        sizes = [up(4 * f, 256) for f in floats]
        total = sum(sizes)
        if route == "mfma":
            sizes[14] = sizes[13]                                             # part2 IS part: counted once
        return route, ld, cq, cs, sizes, total

    def workspace(self, B, N, d, C, sup=0):
        return self.plan(B, N, d, C, sup)[-1]


def uses_split(L, B, N, d, C, sup=0):
    return bool(L.load().nw_bwd_uses_split(B, N, d, C, sup))


def ws_bytes(L, B, N, d, C, sup=0, kind=0):
    return L.load().nw_bwd_workspace_bytes(B, N, d, C, kind, sup)


def held_to(L, rule, B, N, d, C, sup=0):
    """Every answer of the library about one shape against the restated rule; returns the library's plan."""
    route, ld, cq, cs, sizes, total = rule.plan(B, N, d, C, sup)
    p = L.bwd_plan(B, N, d, C, sup)
    where = (rule.split_knob, rule.no_mfma, B, N, d, C, sup)
    assert uses_split(L, B, N, d, C, sup) == rule.split(B, N, d, C, sup) == (route == "split"), where
    assert ws_bytes(L, B, N, d, C, sup) == total == p.total, where
    assert L.BWD_ROUTES[p.route] == route and p.ld == ld and p.Bpad == up(B, 32), where
    assert (p.gq_chunks, p.gs_chunks) == (cq, cs), where
    assert list(p.bytes) == sizes, where
    assert bool(p.parts_shared) == (route == "mfma"), where
    return p


MAP_AREAS = ("A", "Rs", "rq", "gls", "qn2", "sn2", "rs", "s_split", "s_scale", "q_split", "ascale", "qv", "gfac", "part", "part2")


def check_map(L, B, N, d, C, sup=0):
    """The areas in the stated order, on multiples of 256 bytes, each starting where the one before ends and the last ending
    at the total -- hence pairwise disjoint, but for part2 on the fp32 matrix cores, which IS part -- and each at least as
    large as what its user stores there."""
    p = L.bwd_plan(B, N, d, C, sup)
    assert L.BWD_AREAS == MAP_AREAS and len(p.off) == len(p.bytes) == 15
    off, size = dict(zip(MAP_AREAS, p.off)), dict(zip(MAP_AREAS, p.bytes))
    route, where = L.BWD_ROUTES[p.route], (B, N, d, C, sup)
    assert all(o % 256 == 0 for o in p.off) and all(b % 256 == 0 for b in p.bytes), where
    assert off["A"] == 0
    chain = MAP_AREAS[:-1] if p.parts_shared else MAP_AREAS
    for prev, a in zip(chain, chain[1:]):
        assert off[a] == off[prev] + size[prev], (where, a)
    assert off[chain[-1]] + size[chain[-1]] == p.total == ws_bytes(L, B, N, d, C, sup), where
    if p.parts_shared:
        assert route == "mfma" and (off["part2"], size["part2"]) == (off["part"], size["part"]), where
    elif route == "split":
        assert off["part2"] >= off["part"] + size["part"], where
    # what the kernels store: the row stride and the K-splits are the plan's own, held to the rule elsewhere
    ld, cq, cs = p.ld, p.gq_chunks, p.gs_chunks
    assert ld >= N and p.Bpad >= B and p.Bpad % 32 == 0 and ld % {"split": 32, "mfma": 4, "valu": 1}[route] == 0, where
    tail = XGEMM_TAIL if route == "split" else 0
    assert size["A"] >= 4 * (B * ld + tail) and size["Rs"] >= 4 * B * ld, where
    assert min(size["rq"], size["gls"], size["qn2"]) >= 4 * B, where
    assert size["sn2"] >= 4 * (B * N if sup else N), where
    if route == "valu":
        assert (cq, cs) == (0, 0) and all(size[a] == 0 for a in MAP_AREAS[6:]), where
    else:
        assert cq >= 1 and cs >= 1 and size["rs"] >= 4 * N, where
        assert size["part"] >= 4 * cq * B * d * (cq > 1) and size["part2"] >= 4 * cs * N * d * (cs > 1), where
    if route == "split":
        assert size["s_split"] >= 4 * (N * d + tail) and size["s_scale"] >= 4 * N, where
        assert size["q_split"] >= 4 * (p.Bpad * d + tail), where
        assert min(size["ascale"], size["qv"]) >= 4 * B and size["gfac"] >= 4, where
    else:
        assert all(size[a] == 0 for a in MAP_AREAS[7:13]), where
    # the coefficient launch
    assert p.coeff_threads == (1024 if N >= 2048 else 256), where
    assert p.coeff_lds_bytes == 4 * (80 + C + (ld if route == "split" else 0)), where
    assert p.status == (NW_ERR_UNSUPPORTED if p.coeff_lds_bytes > LDS_LAUNCH_BYTES else NW_OK), where
    return p


# the shapes of tests/test_head_backward_gpu.py's edge cases and the route each must take by default
EDGE_TABLE = [
    ((16, 20000, 32, 5), "split"),        # coefficient kernel above 64 KiB of LDS: 80 340 bytes
    ((16, 38300, 32, 16), "split"),       # ld = 38304: 80 + 38304 + 16 = 38400 floats, exactly 150 KiB
    ((16, 38305, 32, 16), "mfma"),        # ld = 38336: one 32-float step past it
    ((8, 300, 16, 20000), "valu"),
    ((64, 1000, 512, 30000), "split"),    # 80 + 1024 + 30000 = 31104 floats: still under the limit
    ((64, 1000, 512, 37500), "mfma"),     # 80 + 1024 + 37500 = 38604: past it
    ((4, 2048, 16, 3), "valu"),
    ((16, 256, 1024, 5), "split"),        # B N d = 2^22 exactly
    ((15, 280, 1024, 5), "mfma"),         # B < 16
    ((16, 255, 1056, 5), "mfma"),         # N < 256
    ((16, 256, 992, 5), "valu"),          # B N d < 2^22
    ((64, 1024, 64, 5), "split"), ((129, 257, 160, 1000), "split"), ((33, 4099, 64, 7), "split"),
]


@pytest.mark.parametrize("shape,route", EDGE_TABLE)
def test_default_route_of_the_edge_shapes(L, knobs, shape, route):
    B, N, d, C = shape
    assert Rule().route(B, N, d, C) == route            # the table agrees with the rule as written down here
    assert uses_split(L, B, N, d, C) == (route == "split")
    assert L.BWD_ROUTES[held_to(L, Rule(), B, N, d, C).route] == route
    knobs(bwd_no_mfma=1)
    assert not uses_split(L, B, N, d, C)
    assert L.BWD_ROUTES[held_to(L, Rule(no_mfma=True), B, N, d, C).route] == "valu"


@pytest.mark.parametrize("C", [0, 1, 16, 1000, 1008, 5000, 20000, 37000, 38000, 38065, 38320, 40000])
def test_lds_boundary_is_a_function_of_ld_plus_classes(L, knobs, C):
    """Largest N that still splits: 80 + ld + C <= 38400 floats, ld = N rounded up to 32 -- both sides, for several C."""
    B, d = 64, 512                                                       # (B N d >= 2^22 from N = 128)
    ld_max = (LDS_SPLIT_FLOATS - 80 - C) // 32 * 32
    if ld_max < 256:                                                     # no N >= 256 fits next to this many classes
        for N in (256, 1024, 38400):
            assert not uses_split(L, B, N, d, C)
        knobs(bwd_split=1)
        assert not uses_split(L, B, 1024, d, C)
        return
    for N, want in ((ld_max - 31, True), (ld_max, True), (ld_max + 1, False), (ld_max + 32, False)):
        assert uses_split(L, B, N, d, C) == want, (N, C)
        assert Rule().split(B, N, d, C) == want
        held_to(L, Rule(), B, N, d, C)
    knobs(bwd_split=1)                                                   # forcing the route does not lift the LDS limit
    assert uses_split(L, B, ld_max, d, C) and not uses_split(L, B, ld_max + 1, d, C)
    # and with one class more at the last fitting ld, when that ld is full
    if 80 + ld_max + C == LDS_SPLIT_FLOATS:
        assert not uses_split(L, B, ld_max, d, C + 1)


THRESHOLD_CASES = [(16, 256, 1024, 5), (15, 280, 1024, 5), (16, 255, 1056, 5), (16, 256, 992, 5), (16, 256, 1020, 5),
             (16, 300, 1008, 5),                      # d % 32 == 16: fp32 matrix cores whatever the knob says
             (16, 300, 1022, 5),                      # d % 4 != 0: VALU
             (2, 4096, 512, 5), (4096, 2, 512, 5), (1, 1, 32, 1), (64, 1024, 64, 5), (63, 1024, 64, 5), (64, 1023, 64, 5),
             (64, 1024, 32, 5), (256, 10000, 512, 200)]
KNOB_STATES = [(s, m) for s in (None, 0, 1) for m in (None, 1)]


def test_thresholds_and_the_three_knob_values(L, knobs):
    cases = THRESHOLD_CASES
    for split_knob in (None, 0, 1):
        for no_mfma in (None, 1):
            knobs(bwd_split=split_knob, bwd_no_mfma=no_mfma)
            rule = Rule(split_knob, no_mfma == 1)
            for B, N, d, C in cases:
                for sup in (0, 1):
                    held_to(L, rule, B, N, d, C, sup)
    # what the knob changes and what it does not
    assert Rule(1).split(15, 280, 1024, 5) and Rule(1).split(16, 255, 1056, 5)      # B and N thresholds: lifted by 1
    assert not Rule(1).split(16, 256, 992, 5)                                        # B N d >= 2^22: never lifted
    assert not Rule(1).split(16, 300, 1008, 5)                                       # d % 32: never lifted
    assert not Rule(0).split(256, 10000, 512, 200)


def test_workspace_moves_across_each_boundary_as_the_layout_says(L, knobs):
    w = lambda *a: ws_bytes(L, *a)
    # VALU -> fp32 matrix cores at B N d = 2^22: rs, the partial tiles, rows padded to 4 floats
    assert w(16, 256, 1020, 5) < w(16, 256, 1024, 5) and w(15, 273, 1024, 5) < w(15, 274, 1024, 5)
    assert Rule().route(15, 273, 1024, 5) == "valu" and Rule().route(15, 274, 1024, 5) == "mfma"
    # fp32 matrix cores -> split at B = 16 and at N = 256: the split images of s and q, both products' partial tiles
    assert w(15, 280, 1024, 5) < w(16, 280, 1024, 5)
    assert w(17, 255, 1024, 5) < w(17, 256, 1024, 5)
    assert Rule().route(17, 255, 1024, 5) == "mfma" and Rule().route(17, 256, 1024, 5) == "split"
    knobs(bwd_split=0)
    off = w(16, 280, 1024, 5)
    knobs(bwd_split=None)
    assert off < w(16, 280, 1024, 5)
    # split -> fp32 matrix cores past the LDS limit: five more supports, and a SMALLER workspace (no split images)
    assert w(16, 38305, 32, 16) < w(16, 38300, 32, 16)
    # per-query supports never leave the VALU route: the norms of B N rows are all that grows
    assert w(16, 256, 1024, 5, 1) == Rule().workspace(16, 256, 1024, 5, 1) == Rule(no_mfma=True).workspace(16, 256, 1024, 5) \
        + up(4 * 16 * 256, 256) - up(4 * 256, 256)
    # the class count is no part of any buffer: it only moves the route
    assert w(64, 1000, 512, 37500) < w(64, 1000, 512, 30000) and w(8, 300, 16, 1) == w(8, 300, 16, 20000)


def test_sizes_of_empty_and_negative_batches_are_zero(L, knobs):
    for B in (0, -1, -2 ** 40):
        for N in (0, 1, 1000, 38300):
            for sup in (0, 1):
                assert ws_bytes(L, B, N, 64, 5, sup) == 0
                assert not uses_split(L, B, N, 64, 5, sup)
    assert ws_bytes(L, 16, -1, 64, 5) == 0
    for bad in ((16, 0, 64, 5), (16, 1000, 0, 5), (16, 1000, 64, -1), (16, -5, 64, 5)):
        assert not uses_split(L, *bad)
    assert ws_bytes(L, 1, 0, 64, 5) == Rule().workspace(1, 0, 64, 5)      # an empty support set: five (empty or one-float) buffers


@pytest.mark.parametrize("split_knob,no_mfma", KNOB_STATES)
def test_areas_tile_the_workspace_and_hold_what_is_stored_there(L, knobs, split_knob, no_mfma):
    knobs(bwd_split=split_knob, bwd_no_mfma=no_mfma)
    rule, seen = Rule(split_knob, no_mfma == 1), set()
    for B, N, d, C in [s for s, _ in EDGE_TABLE] + THRESHOLD_CASES + [(2, 30, 8, 40880), (2, 30, 8, 40881), (256, 512, 64, 5)]:
        for sup in (0, 1):
            p = check_map(L, B, N, d, C, sup)
            assert list(p.bytes) == rule.plan(B, N, d, C, sup)[4]
            seen.add((L.BWD_ROUTES[p.route], p.gq_chunks > 1, p.gs_chunks > 1))
    if split_knob is None and no_mfma is None:                                # all three routes, both products split and unsplit
        assert {r for r, _, _ in seen} == {"valu", "mfma", "split"}
        assert {("split", True, True), ("split", True, False)} <= seen
    if split_knob == 0 and no_mfma is None:
        assert ("mfma", True, True) in seen
    p = check_map(L, 256, 512, 64, 5)
    off, size = dict(zip(MAP_AREAS, p.off)), dict(zip(MAP_AREAS, p.bytes))
    if L.BWD_ROUTES[p.route] == "split":                                      # both live at once: disjoint
        assert size["part"] > 0 and size["part2"] > 0 and off["part"] + size["part"] <= off["part2"]
    elif L.BWD_ROUTES[p.route] == "mfma":                                     # one buffer, sized for the larger
        assert (off["part"], size["part"]) == (off["part2"], size["part2"]) and size["part"] >= 4 * max(8 * 256 * 64, 4 * 512 * 64)


def test_xgemm_wgs_moves_the_k_split_of_the_split_route_only(L, knobs):
    for wgs in (64, 1024):
        knobs(xgemm_wgs=wgs)
        for B, N, d, C in ((64, 1024, 64, 5), (256, 512, 64, 5), (256, 10000, 512, 200), (15, 280, 1024, 5), (8, 300, 16, 5)):
            held_to(L, Rule(xgemm_wgs=wgs), B, N, d, C)
            check_map(L, B, N, d, C)
    knobs(xgemm_wgs=64)
    few = L.bwd_plan(256, 10000, 512, 200).gq_chunks
    knobs(xgemm_wgs=None)
    assert few < L.bwd_plan(256, 10000, 512, 200).gq_chunks == 16


def test_totals_and_split_answers_are_those_of_the_library_before_the_plan(L, knobs):
    """tests/golden/bwd_workspace_bytes.npz (record_bwd_workspace_bytes.py, from the parent of the plan): exactly."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "bwd_workspace_bytes.npz"))
    lib = L.load()

    def replay(shapes, total, split, what):
        assert len(shapes) == len(total) == len(split)
        for (B, N, d, C, sup), t, s in zip(shapes.tolist(), total.tolist(), split.tolist()):
            assert lib.nw_bwd_workspace_bytes(B, N, d, C, 0, sup) == t, (what, B, N, d, C, sup)
            assert lib.nw_bwd_uses_split(B, N, d, C, sup) == s, (what, B, N, d, C, sup)
            p = L.bwd_plan(B, N, d, C, sup)
            assert p.total == t and (p.route == 2) == bool(s), (what, B, N, d, C, sup)
    assert len(z["shapes"]) == 5040 and len(z["sub_shapes"]) == 360 and len(z["knob_states"]) == 7
    replay(z["shapes"], z["total"], z["split"], "default")
    for i, (sk, nm, wgs) in enumerate(z["knob_states"].tolist()):
        knobs(bwd_split=sk, bwd_no_mfma=nm, xgemm_wgs=wgs)
        replay(z["sub_shapes"], z[f"total_k{i}"], z[f"split_k{i}"], (sk, nm, wgs))


def test_refused_arguments_and_empty_batches_of_the_plan(L):
    import ctypes
    lib, p = L.load(), L.BwdPlan()
    assert lib.nw_debug_bwd_plan(64, 1024, 64, 5, 0, None) == NW_ERR_INVALID_ARG
    for bad in ((-1, 1024, 64, 5), (64, -1, 64, 5), (64, 1024, -64, 5), (64, 1024, 64, -5)):
        assert lib.nw_debug_bwd_plan(*bad, 0, ctypes.byref(p)) == NW_ERR_INVALID_ARG
    for sup in (0, 1):
        ctypes.memset(ctypes.byref(p), 0xFF, ctypes.sizeof(p))
        assert lib.nw_debug_bwd_plan(0, 1024, 64, 5, sup, ctypes.byref(p)) == NW_OK
        assert bytes(p) == bytes(ctypes.sizeof(p))
    assert ctypes.sizeof(p) == 8 * 4 + 3 * 8 + 2 * 15 * 8 + 8


def test_sanitizer_program_builds_and_exits_0():
    """tests/sanitize/abi_args_bwd.cpp: the plan over the edge shapes and every refusal of the backward's entries that
    returns before a launch, as a stand-alone host-only AddressSanitizer + UndefinedBehaviorSanitizer build of the library's
    own sources against a HIP runtime stand-in; nothing is loaded into python."""
    import subprocess
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "nwhead_amd", "csrc"), "sanitize_bwd", "-j4"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    assert "abi_args_bwd: all argument checks refused as documented" in r.stdout
    assert "runtime error" not in r.stdout + r.stderr and "AddressSanitizer" not in r.stdout + r.stderr
