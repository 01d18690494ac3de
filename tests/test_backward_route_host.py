"""Which of its three product routes the head's backward takes, and how much workspace it asks for, on the host: no GPU.

The expected values are NOT read back from the library: `Rule` below restates DESIGN.md 4.6 (the route rule) and the layout of
backward.hip's `bwd_layout` (the buffers each route needs), and the library is held to it.
  VALU    everything else
  fp32 matrix cores   shared supports, d % 4 == 0, B N d >= 2^22, unless bwd_no_mfma = 1
  split fp16          the above and d % 32 == 0 and (80 + ld + C) floats <= 150 KiB with ld = N rounded up to 32
                      and, unless bwd_split = 1, B >= 16 and N >= 256; never with bwd_split = 0
"""
import pytest

UNSET = -2 ** 31
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
    """DESIGN.md 4.6, restated."""

    def __init__(self, split_knob=None, no_mfma=False):
        self.split_knob, self.no_mfma = split_knob, no_mfma

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

    def workspace(self, B, N, d, C, sup=0):
        """bwd_layout: every buffer a whole number of 256-byte units."""
        route = self.route(B, N, d, C, sup)
        ld = up(N, 32) if route == "split" else up(N, 4) if route == "mfma" else N
        a = lambda nfloat: up(4 * nfloat, 256)
        total = a(B * ld + (XGEMM_TAIL if route == "split" else 0)) + a(B * ld) + 3 * a(B) + a(B * N if sup else N)
        if route == "valu":
            return total
        total += a(N)                                                     # rs
        if route == "split":
            cq = self._chunks(B, d, N, 128, 64, 32, 256, 128)             # first product: M = B, K = N
            cs = self._chunks(N, d, B, 128, 64, 32, 256, 128)             # second product: M = N, K = B
            total += a(N * d + XGEMM_TAIL) + a(N) + a(up(B, 32) * d + XGEMM_TAIL) + 2 * a(B) + a(1)
            return total + a(cq * B * d if cq > 1 else 0) + a(cs * N * d if cs > 1 else 0)
        cq = self._chunks(B, d, N, 128, 128, 16, 512, 64)
        cs = self._chunks(N, d, B, 128, 128, 16, 512, 64)
        return total + a(max(cq * B * d if cq > 1 else 0, cs * N * d if cs > 1 else 0))


def uses_split(L, B, N, d, C, sup=0):
    return bool(L.load().nw_bwd_uses_split(B, N, d, C, sup))


def ws_bytes(L, B, N, d, C, sup=0, kind=0):
    return L.load().nw_bwd_workspace_bytes(B, N, d, C, kind, sup)


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
    assert ws_bytes(L, B, N, d, C) == Rule().workspace(B, N, d, C)
    knobs(bwd_no_mfma=1)
    assert not uses_split(L, B, N, d, C)
    assert ws_bytes(L, B, N, d, C) == Rule(no_mfma=True).workspace(B, N, d, C)


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
        assert ws_bytes(L, B, N, d, C) == Rule().workspace(B, N, d, C)
    knobs(bwd_split=1)                                                   # forcing the route does not lift the LDS limit
    assert uses_split(L, B, ld_max, d, C) and not uses_split(L, B, ld_max + 1, d, C)
    # and with one class more at the last fitting ld, when that ld is full
    if 80 + ld_max + C == LDS_SPLIT_FLOATS:
        assert not uses_split(L, B, ld_max, d, C + 1)


def test_thresholds_and_the_three_knob_values(L, knobs):
    cases = [(16, 256, 1024, 5), (15, 280, 1024, 5), (16, 255, 1056, 5), (16, 256, 992, 5), (16, 256, 1020, 5),
             (16, 300, 1008, 5),                      # d % 32 == 16: fp32 matrix cores whatever the knob says
             (16, 300, 1022, 5),                      # d % 4 != 0: VALU
             (2, 4096, 512, 5), (4096, 2, 512, 5), (1, 1, 32, 1), (64, 1024, 64, 5), (63, 1024, 64, 5), (64, 1023, 64, 5),
             (64, 1024, 32, 5), (256, 10000, 512, 200)]
    for split_knob in (None, 0, 1):
        for no_mfma in (None, 1):
            knobs(bwd_split=split_knob, bwd_no_mfma=no_mfma)
            rule = Rule(split_knob, no_mfma == 1)
            for B, N, d, C in cases:
                for sup in (0, 1):
                    assert uses_split(L, B, N, d, C, sup) == rule.split(B, N, d, C, sup), (split_knob, no_mfma, B, N, d, C, sup)
                    assert ws_bytes(L, B, N, d, C, sup) == rule.workspace(B, N, d, C, sup), (split_knob, no_mfma, B, N, d, C, sup)
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
