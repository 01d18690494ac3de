"""The host-side surface of the query gradient over a resident bank (no GPU): nw_bwd_query_f32's declaration and refusals
through ctypes, the stand-alone sanitizer program of the entry (tests/sanitize/abi_args_bwd_query.cpp: host-only
AddressSanitizer + UndefinedBehaviorSanitizer build of the library's own sources against a HIP runtime stand-in; nothing is
loaded into python), the two workspace conditions, the route rule as a table, and the refusals of ops.nw_head_bank and
NWNet.forward_bank."""
import ctypes
import os
import subprocess

import pytest
import torch

NW_OK, NW_ERR_INVALID_ARG, NW_ERR_UNSUPPORTED, NW_ERR_WORKSPACE = 0, -1, -2, -3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from nwhead_amd import _lib
    return _lib


def test_declaration_and_signature():
    text = open(os.path.join(ROOT, "include", "nwhead_hip.h")).read()
    assert "int nw_bwd_query_f32(" in text and "size_t nw_bwd_query_workspace_bytes(" in text
    assert "#define NW_ABI_VERSION 2" in text.replace("  ", " ")
    assert len(_lib().SIGNATURES["nw_bwd_query_f32"][1]) == 23
    assert len(_lib().SIGNATURES["nw_bwd_query_workspace_bytes"][1]) == 5
    assert _lib().load().nw_abi_version() == 2


def test_sanitizer_program_builds_and_exits_0():
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "nwhead_amd", "csrc"), "sanitize_bwd_query", "-j4"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    assert "abi_args_bwd_query: all argument checks refused as documented" in r.stdout
    assert "runtime error" not in r.stdout + r.stderr and "AddressSanitizer" not in r.stdout + r.stderr


def _aligned(nbytes):
    raw = ctypes.create_string_buffer(nbytes + 16)
    return raw, (ctypes.addressof(raw) + 15) & ~15


def test_refusals_before_any_launch():
    lib = _lib().load()
    B, N, d, C = 8, 1000, 64, 5
    need = lib.nw_bwd_query_workspace_bytes(B, N, d, C, 0)
    assert need > 0
    keep, buf = _aligned(256)           # stands for every device pointer: a refused call reads none of them

    def call(q=buf, s=buf, scale=buf, n2=buf, sy=buf, lo=buf, hi=buf, exclude=0, lse=buf, out=buf, gout=buf, gq=buf, gls=None,
             ws=buf, ws_bytes=need - 1, B=B, N=N, d=d, C=C, kind=0, ls=None, chunks=0):
        return lib.nw_bwd_query_f32(q, s, scale, n2, sy, lo, hi, exclude, lse, out, gout, gq, gls, ws, ws_bytes, B, N, d, C, kind,
                                    ls, chunks, None)

    for win in ({}, {"lo": None, "hi": None}):                  # with a window and without
        for name in ("q", "s", "scale", "n2", "sy", "lse", "out", "gout", "gq"):
            assert call(**win, **{name: None}) == NW_ERR_INVALID_ARG, name
        assert call(**win, B=-1) == NW_ERR_INVALID_ARG
        assert call(**win, N=-1) == NW_ERR_INVALID_ARG
        assert call(**win, d=-64) == NW_ERR_INVALID_ARG
        assert call(**win, C=-1) == NW_ERR_INVALID_ARG
        assert call(**win, chunks=-1) == NW_ERR_INVALID_ARG
        assert call(**win, kind=4) == NW_ERR_INVALID_ARG        # clip without its logit scale
        assert call(**win, kind=7) == NW_ERR_UNSUPPORTED
        assert call(**win, d=100) == NW_ERR_UNSUPPORTED         # outside nw_fwd_window_f32's regime
        assert call(**win, d=16) == NW_ERR_UNSUPPORTED
        assert call(**win, d=0) == NW_ERR_UNSUPPORTED
        assert call(**win, N=25) == NW_ERR_UNSUPPORTED
        assert call(**win, C=0) == NW_ERR_UNSUPPORTED
        assert call(**win, q=buf + 4, ws_bytes=need) == NW_ERR_UNSUPPORTED
        assert call(**win, s=buf + 4, ws_bytes=need) == NW_ERR_UNSUPPORTED
        assert call(**win, gq=buf + 8, ws_bytes=need) == NW_ERR_UNSUPPORTED
        assert call(**win, ws=buf + 4, ws_bytes=need) == NW_ERR_UNSUPPORTED
        assert call(**win) == NW_ERR_WORKSPACE                  # short workspace
        assert call(**win, ws=None, ws_bytes=need) == NW_ERR_WORKSPACE
        assert call(**win, ws_bytes=0) == NW_ERR_WORKSPACE
        assert call(**win, B=0) == NW_OK
    assert call(lo=None) == NW_ERR_INVALID_ARG                   # one half of a window
    assert call(hi=None) == NW_ERR_INVALID_ARG
    assert call(lo=None, B=0) == NW_ERR_INVALID_ARG
    assert call(B=0, q=None, s=None, sy=None, out=None, gq=None, ws=None, ws_bytes=0) == NW_OK
    # a shape outside the regime has no workspace
    for shape in ((8, 1000, 100, 5), (8, 25, 64, 5), (8, 1000, 64, 0), (0, 1000, 64, 5), (8, 1000, 16, 5)):
        assert lib.nw_bwd_query_workspace_bytes(*shape, 0) == 0, shape
    # more chunks, more partial tiles; clamped at the tile count
    sizes = [lib.nw_bwd_query_workspace_bytes(33, 4099, 64, 7, c) for c in (1, 2, 3, 7, 4099, 10 ** 6)]
    assert sizes == sorted(sizes) and sizes[0] < sizes[3] and sizes[4] == sizes[5]
    del keep


def test_workspace_conditions():
    """A condition, not a measurement: at the two shapes of the measurement the workspace stays below a quarter of one score
    matrix (B N bytes) and does not more than double from N / 2 to N."""
    lib = _lib().load()
    for B, N, d, C in ((256, 50000, 512, 200), (256, 400000, 256, 200)):
        full, half = lib.nw_bwd_query_workspace_bytes(B, N, d, C, 0), lib.nw_bwd_query_workspace_bytes(B, N // 2, d, C, 0)
        assert 0 < full < B * N, (full, B * N)
        assert 0 < half and full <= 2 * half, (full, half)


def test_route_rule():
    from nwhead_amd.ops import HEAD_WINDOW_MAX_CLASSES, head_bank_refusal, head_bank_route, head_window_route
    base = dict(split=True, sorted_copy=False, shape=(50000, 512), pad=0, width=512, B=256, n_classes=200)
    table = [
        ({}, "fused", None),
        ({"shape": (26, 32), "width": 32, "B": 1, "n_classes": 1}, "fused", None),        # no size gate
        ({"pad": 12, "width": 500}, "fused", None),                                         # a padded bank
        ({"n_classes": HEAD_WINDOW_MAX_CLASSES}, "fused", None),
        ({"split": False}, "matrix", "no split rows"),                                      # fp16 or norms-only bank
        ({"sorted_copy": True}, "matrix", "unsorted labels"),
        ({"shape": (25, 512)}, "matrix", "25 rows"),
        ({"width": 500}, "matrix", "do not pad"),
        ({"shape": (50000, 500), "width": 500}, "matrix", "multiple of 32"),
        ({"n_classes": 0}, "matrix", "classes"),
        ({"n_classes": HEAD_WINDOW_MAX_CLASSES + 1}, "matrix", "classes"),
        ({"B": 0}, "matrix", "empty"),
    ]
    for change, route, why in table:
        facts = {**base, **change}
        assert head_bank_route(**facts) == route, change
        assert head_bank_route(**facts) == head_window_route(**facts), change               # the windowed forward's own rule
        reason = head_bank_refusal(**facts)
        assert (reason is None) if why is None else (why in reason), (change, reason)


class _AnyBank:
    label_max = None

    def matches(self, s):
        return True


def test_nw_head_bank_refusals():
    from nwhead_amd import ops
    q, s, sy = torch.zeros(4, 64, requires_grad=True), torch.zeros(100, 64), torch.zeros(100, dtype=torch.int64)
    with pytest.raises(TypeError, match="prepared bank"):
        ops.nw_head_bank(q, s, sy, 5, None)
    with pytest.raises(TypeError, match="prepared bank"):
        ops.nw_head_bank(q, s, sy, 5, _AnyBank())
    bank = ops.SplitBank.__new__(ops.SplitBank)     # stands for a prepared bank: the refusals below come before it is used
    with pytest.raises(ValueError, match="constant.*nw_head"):
        ops.nw_head_bank(q, s.clone().requires_grad_(True), sy, 5, bank)
    with pytest.raises(ops.NWHipError, match="MI355X"):        # no CPU route: the device's refusal
        ops.nw_head_bank(q, s, sy, 5, bank)


def test_nwnet_forward_bank_refusals():
    from test_sharded_knn_host import _net
    from nwhead_amd.ops import NWHipError
    x = torch.zeros(2, 3, 4, 4)
    rows = torch.tensor([0, -1])
    net = _net()
    for leave in (None, rows):
        with pytest.raises(NWHipError, match="forward_bank needs the bank of precompute"):
            net.forward_bank(x, leave_out=leave)
    hook = lambda *a: None  # noqa: E731  (the compute hooks of the CPU tests: nothing is computed here)
    with torch.no_grad():
        net.precompute_sharded(partial_fn=hook, merge_fn=hook, search_fn=hook, knn_merge_fn=hook)
    for leave in (None, rows):
        with pytest.raises(NWHipError, match="forward_bank: a sharded bank"):
            net.forward_bank(x, leave_out=leave)
    net = _net()
    net.full_feat, net.full_y = torch.zeros(70, 16), torch.zeros(70, dtype=torch.int64)
    net.kernel = torch.nn.Identity()                # a custom kernel module
    with pytest.raises(NWHipError, match="built-in score kernels"):
        net.forward_bank(x)
