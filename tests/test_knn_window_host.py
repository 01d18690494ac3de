"""The windowed neighbour search's host-side surface (no GPU): the stand-alone sanitizer program of the two new entries
(tests/sanitize/abi_args_knn_window.cpp: host-only AddressSanitizer + UndefinedBehaviorSanitizer build of the library's own
sources against a HIP runtime stand-in; nothing is loaded into python), the workspace of nw_knn_window_f32, the
monotonicity argument that ops.nw_top_influence rests on, and NWNet.explain's refusal of a sharded bank."""
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


def test_status_codes_are_the_headers():
    text = open(os.path.join(ROOT, "include", "nwhead_hip.h")).read()
    for name, value in (("NW_ERR_INVALID_ARG", NW_ERR_INVALID_ARG), ("NW_ERR_UNSUPPORTED", NW_ERR_UNSUPPORTED),
                        ("NW_ERR_WORKSPACE", NW_ERR_WORKSPACE)):
        assert f"{name} = {value}," in text, name


def test_sanitizer_program_builds_and_exits_0():
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "nwhead_amd", "csrc"), "sanitize_knn_window", "-j4"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    assert "abi_args_knn_window: all argument checks refused as documented" in r.stdout
    assert "runtime error" not in r.stdout + r.stderr and "AddressSanitizer" not in r.stdout + r.stderr


def _aligned(nbytes):
    raw = ctypes.create_string_buffer(nbytes + 16)
    return raw, (ctypes.addressof(raw) + 15) & ~15


def test_workspace_is_nw_knn_f32s_and_is_checked_before_any_launch():
    lib = _lib().load()
    B, N, d, k = 8, 1000, 64, 10
    need = lib.nw_knn_workspace_bytes(B, N, d, k)
    assert need > 0
    keep, buf = _aligned(256)           # stands for every device pointer: a refused call reads none of them

    def call(ws, ws_bytes, exclude=0, lo=buf, hi=buf):
        return lib.nw_knn_window_f32(buf, buf, buf, buf, lo, hi, exclude, buf, None, ws, ws_bytes, B, N, d, k, 0, None, None)

    for exclude in (0, 1):
        assert call(buf, need - 1, exclude) == NW_ERR_WORKSPACE
        assert call(None, need, exclude) == NW_ERR_WORKSPACE
        assert call(buf, 0, exclude) == NW_ERR_WORKSPACE
    assert call(buf, need - 1, lo=None) == NW_ERR_INVALID_ARG
    assert call(buf, need - 1, hi=None) == NW_ERR_INVALID_ARG
    assert call(buf + 4, need) == NW_ERR_INVALID_ARG            # workspace not 16-byte aligned
    # the same check, in the same place, as the search without a window
    assert lib.nw_knn_f32(buf, buf, buf, buf, buf, None, buf, need - 1, B, N, d, k, 0, None, None) == NW_ERR_WORKSPACE
    del keep


def test_influence_select_refusals():
    lib = _lib().load()
    keep, buf = _aligned(256)
    f = lib.nw_influence_select_f32
    assert f(buf, buf, buf, buf, buf, buf, buf, None, 4, 0, 100, 5, None) == NW_ERR_UNSUPPORTED
    assert f(buf, buf, buf, buf, buf, buf, buf, None, 4, 33, 100, 5, None) == NW_ERR_UNSUPPORTED
    assert f(buf, buf, buf, buf, buf, buf, buf, None, -1, 10, 100, 5, None) == NW_ERR_INVALID_ARG
    assert f(buf, None, buf, buf, buf, buf, buf, None, 4, 10, 100, 5, None) == NW_ERR_INVALID_ARG
    assert f(buf, buf, buf, buf, buf, buf, buf, buf, 0, 10, 100, 5, None) == NW_OK
    del keep


def test_sorting_a_class_by_weight_sorts_its_influences():
    """infl = log((p - p w) / (p - w [same])) in fp64 on random p and w: over the supports of the query's class it is
    >= 0 and strictly increasing in w (w < p: a support's weight is part of its class's probability), over the others it is
    log(1 - w): <= 0 and strictly decreasing.  So the k best-scoring rows of a class, best first, are its k largest
    influences in non-increasing order, and the k best-scoring rows of the other classes are the k smallest influences in
    non-decreasing order."""
    g = torch.Generator().manual_seed(0)
    for _ in range(50):
        p = torch.rand((), generator=g, dtype=torch.float64) * 0.98 + 0.01
        w_same = torch.rand(64, generator=g, dtype=torch.float64) * p * 0.999
        w_other = torch.rand(64, generator=g, dtype=torch.float64) * (1 - p) * 0.999
        same = torch.log((p - p * w_same) / (p - w_same))
        other = torch.log((p - p * w_other) / p)
        assert bool((same >= 0).all()) and bool((other <= 0).all())
        assert torch.equal(torch.argsort(w_same, descending=True), torch.argsort(same, descending=True))
        assert torch.equal(torch.argsort(w_other, descending=True), torch.argsort(other))
        d_same = same[torch.argsort(w_same)]
        d_other = other[torch.argsort(w_other)]
        assert bool((d_same[1:] > d_same[:-1]).all()) and bool((d_other[1:] < d_other[:-1]).all())


def test_explain_refuses_a_sharded_bank():
    from test_sharded_knn_host import _net
    from nwhead_amd.ops import NWHipError
    net = _net()
    hook = lambda *a: None  # noqa: E731  (the compute hooks of the CPU tests: nothing is computed here)
    with torch.no_grad():
        bank = net.precompute_sharded(partial_fn=hook, merge_fn=hook, search_fn=hook, knn_merge_fn=hook)
    assert bank is net.sharded_bank and not hasattr(net, "full_feat")
    x = torch.zeros(2, 3, 4, 4)
    with pytest.raises(NWHipError, match="sharded"):
        net.explain(x, torch.zeros(2, dtype=torch.int64))
    with pytest.raises(NWHipError, match="precompute"):
        _net().explain(x, torch.zeros(2, dtype=torch.int64))
