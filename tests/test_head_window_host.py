"""The windowed head's host-side surface (no GPU): nw_fwd_window_f32's refusals through ctypes, the stand-alone sanitizer
program of the entry (tests/sanitize/abi_args_fwd_window.cpp: host-only AddressSanitizer + UndefinedBehaviorSanitizer build
of the library's own sources against a HIP runtime stand-in; nothing is loaded into python), the route rule as a pure
function, and the refusals of ops.nw_head(row_window=...) and NWNet.predict(leave_out=...) / predict_loo."""
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


def test_status_codes_and_declaration_are_the_headers():
    text = open(os.path.join(ROOT, "include", "nwhead_hip.h")).read()
    for name, value in (("NW_ERR_INVALID_ARG", NW_ERR_INVALID_ARG), ("NW_ERR_UNSUPPORTED", NW_ERR_UNSUPPORTED),
                        ("NW_ERR_WORKSPACE", NW_ERR_WORKSPACE)):
        assert f"{name} = {value}," in text, name
    assert "int nw_fwd_window_f32(" in text and "#define NW_ABI_VERSION 2" in text.replace("  ", " ")
    assert len(_lib().SIGNATURES["nw_fwd_window_f32"][1]) == 19


def test_sanitizer_program_builds_and_exits_0():
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "nwhead_amd", "csrc"), "sanitize_fwd_window", "-j4"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    assert "abi_args_fwd_window: all argument checks refused as documented" in r.stdout
    assert "runtime error" not in r.stdout + r.stderr and "AddressSanitizer" not in r.stdout + r.stderr


def _aligned(nbytes):
    raw = ctypes.create_string_buffer(nbytes + 16)
    return raw, (ctypes.addressof(raw) + 15) & ~15


def test_refusals_before_any_launch():
    lib = _lib().load()
    B, N, d, C = 8, 1000, 64, 5
    need = lib.nw_fwd_workspace_bytes(B, N, d, C)
    assert need > 0
    keep, buf = _aligned(256)           # stands for every device pointer: a refused call reads none of them

    def call(lo=buf, hi=buf, sy=buf, out=buf, ws=buf, ws_bytes=need - 1, B=B, N=N, d=d, C=C, exclude=0, q=buf, kind=0):
        return lib.nw_fwd_window_f32(q, buf, buf, buf, sy, lo, hi, exclude, out, None, ws, ws_bytes, B, N, d, C, kind, None, None)

    for exclude in (0, 1):
        assert call(lo=None, exclude=exclude) == NW_ERR_INVALID_ARG          # null windows
        assert call(hi=None, exclude=exclude) == NW_ERR_INVALID_ARG
        assert call(lo=None, hi=None, B=0, exclude=exclude) == NW_ERR_INVALID_ARG
        assert call(d=100, exclude=exclude) == NW_ERR_UNSUPPORTED            # outside nw_knn_window_f32's regime
        assert call(N=25, exclude=exclude) == NW_ERR_UNSUPPORTED
        assert call(q=buf + 4, ws_bytes=need, exclude=exclude) == NW_ERR_UNSUPPORTED
        assert call(exclude=exclude) == NW_ERR_WORKSPACE                     # short workspace
        assert call(ws=None, ws_bytes=need, exclude=exclude) == NW_ERR_WORKSPACE
        assert call(ws_bytes=0, exclude=exclude) == NW_ERR_WORKSPACE
        assert call(B=0, exclude=exclude) == NW_OK
        assert call(B=0, q=None, sy=None, out=None, ws=None, ws_bytes=0, exclude=exclude) == NW_OK
    assert call(sy=None) == NW_ERR_INVALID_ARG
    assert call(out=None) == NW_ERR_INVALID_ARG
    assert call(q=None) == NW_ERR_INVALID_ARG
    assert call(B=-1) == NW_ERR_INVALID_ARG
    assert call(N=-1) == NW_ERR_INVALID_ARG
    assert call(C=-1) == NW_ERR_INVALID_ARG
    assert call(kind=4) == NW_ERR_INVALID_ARG                                # clip without its logit scale
    assert call(kind=7) == NW_ERR_UNSUPPORTED
    # the workspace is nw_fwd_f32's: the same size is asked of the plain call
    assert lib.nw_fwd_f32(buf, buf, buf, buf, buf, buf, buf, None, None, None, buf, need - 1, B, N, d, C, 0, None, 0, 0, None,
                          None) == NW_ERR_WORKSPACE
    del keep


def test_the_debug_plan_still_takes_outputs_0_to_2_only():
    """OUT_WIN is 4 (the build check counts the kernels whose third template argument is 2 or 3): nw_debug_fwd_plan's range
    is what it was."""
    lib = _lib()
    for name in ("log_probs", "scores", "candidates"):
        assert lib.fwd_plan(256, 50000, 512, 200, outputs=name, k=10 if name == "candidates" else 0).status == NW_OK
    p = lib.FwdPlan()
    for outputs in (3, 4):
        assert lib.load().nw_debug_fwd_plan(256, 50000, 512, 200, 1, outputs, 0, 1, 0, 0, 256, ctypes.byref(p)) == NW_ERR_INVALID_ARG


def test_route_rule():
    from nwhead_amd.ops import HEAD_WINDOW_MAX_CLASSES, head_window_route
    base = dict(split=True, sorted_copy=False, shape=(50000, 512), pad=0, width=512, B=256, n_classes=200)
    assert head_window_route(**base) == "fused"
    # no size gate: the smallest shapes the kernel takes are fused too
    assert head_window_route(**{**base, "shape": (26, 32), "width": 32, "B": 1, "n_classes": 1}) == "fused"
    assert head_window_route(**{**base, "shape": (50000, 512), "pad": 12, "width": 500}) == "fused"       # a padded bank
    assert head_window_route(**{**base, "split": False}) == "matrix"              # fp16 or norms-only bank
    assert head_window_route(**{**base, "sorted_copy": True}) == "matrix"         # built from unsorted labels
    assert head_window_route(**{**base, "shape": (25, 512)}) == "matrix"          # N <= 25
    assert head_window_route(**{**base, "width": 500}) == "matrix"                # queries that do not pad to the bank
    assert head_window_route(**{**base, "B": 0}) == "matrix"
    assert head_window_route(**{**base, "n_classes": 0}) == "matrix"
    assert head_window_route(**{**base, "n_classes": HEAD_WINDOW_MAX_CLASSES}) == "fused"
    assert head_window_route(**{**base, "n_classes": HEAD_WINDOW_MAX_CLASSES + 1}) == "matrix"
    # the class limit is the library's: the entry refuses one class more before anything is launched
    lib = _lib().load()
    keep, buf = _aligned(256)
    f = lambda C: lib.nw_fwd_window_f32(buf, buf, buf, buf, buf, buf, buf, 0, buf, None, buf, 0, 8, 1000, 64, C, 0, None, None)  # noqa: E731
    assert f(HEAD_WINDOW_MAX_CLASSES) == NW_ERR_WORKSPACE and f(HEAD_WINDOW_MAX_CLASSES + 1) == NW_ERR_UNSUPPORTED
    del keep


class _AnyBank:
    """Stands for a prepared bank of whatever tensor it is asked about (the refusals below come before it is used)."""
    label_max = None

    def matches(self, s):
        return True


def test_nw_head_refuses_what_the_window_cannot_serve():
    from nwhead_amd import ops
    q, s, sy = torch.zeros(4, 64), torch.zeros(100, 64), torch.zeros(100, dtype=torch.int64)
    win = (torch.zeros(4, dtype=torch.int64), torch.ones(4, dtype=torch.int64))
    with pytest.raises(ValueError, match="support_cache"):
        ops.nw_head(q, s, sy, 5, row_window=win)                                              # no bank
    with pytest.raises(ValueError, match="no gradients"):
        ops.nw_head(q.clone().requires_grad_(True), s, sy, 5, support_cache=_AnyBank(), row_window=win)
    with pytest.raises(ValueError, match="no gradients"):
        ops.nw_head(q, s.clone().requires_grad_(True), sy, 5, support_cache=_AnyBank(), row_window=win)
    with pytest.raises(ValueError, match="return_weights"):
        ops.nw_head(q, s, sy, 5, return_weights=True, support_cache=_AnyBank(), row_window=win, exclude=True)
    with torch.no_grad():                                       # without gradients the refusal is the device's, not this one
        with pytest.raises(ops.NWHipError, match="MI355X"):
            ops.nw_head(q.clone().requires_grad_(True), s, sy, 5, support_cache=_AnyBank(), row_window=win)


def test_nwnet_refusals():
    from test_sharded_knn_host import _net
    from nwhead_amd.ops import NWHipError
    x = torch.zeros(2, 3, 4, 4)
    rows = torch.tensor([0, -1])
    net = _net()
    for mode in ("random", "knn", "ensemble", "cluster"):
        with pytest.raises(NWHipError, match="only mode='full'"):
            net.predict(x, mode, leave_out=rows)
    with pytest.raises(NWHipError, match="precompute"):
        net.predict(x, "full", leave_out=rows)
    with pytest.raises(NWHipError, match="precompute"):
        net.predict_loo()
    hook = lambda *a: None  # noqa: E731  (the compute hooks of the CPU tests: nothing is computed here)
    with torch.no_grad():
        net.precompute_sharded(partial_fn=hook, merge_fn=hook, search_fn=hook, knn_merge_fn=hook)
    with pytest.raises(NWHipError, match="sharded"):
        net.predict(x, "full", leave_out=rows)
    with pytest.raises(NWHipError, match="sharded"):
        net.predict_loo(rows=torch.tensor([1, 2]))
