"""The host-side surface of the value head's gradients to the values and the support weights (no GPU): the declarations and
refusals of nw_bwd_values_support_f32 / nw_bwd_values_support_workspace_bytes through ctypes, their stand-alone sanitizer
program (tests/sanitize/abi_args_bwd_values_support.cpp: a host-only AddressSanitizer + UndefinedBehaviorSanitizer build of the
library's own sources against a HIP runtime stand-in; nothing is loaded into python), the kernel unit's no-scratch rule of the
Makefile, and the refusals of ops.nw_head_values_bank that the new keyword leaves as they were."""
import ctypes
import inspect
import os
import subprocess

import pytest
import torch

NW_OK, NW_ERR_INVALID_ARG, NW_ERR_UNSUPPORTED, NW_ERR_WORKSPACE = 0, -1, -2, -3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nwhead_amd", "csrc")


def _lib():
    from nwhead_amd import _lib
    return _lib


def test_declarations_are_the_headers():
    text = open(os.path.join(ROOT, "include", "nwhead_hip.h")).read()
    assert "int nw_bwd_values_support_f32(" in text and "size_t nw_bwd_values_support_workspace_bytes(" in text
    assert "#define NW_ABI_VERSION 2" in text.replace("  ", " ")
    assert "|error of gvalues[j,t]|" in text                    # the error bound is written down
    sig = _lib().SIGNATURES
    assert len(sig["nw_bwd_values_support_f32"][1]) == 24 and len(sig["nw_bwd_values_support_workspace_bytes"][1]) == 6
    assert sig["nw_bwd_values_support_workspace_bytes"][0] is ctypes.c_size_t
    lib = _lib().load()
    assert hasattr(lib, "nw_bwd_values_support_f32") and hasattr(lib, "nw_bwd_values_support_workspace_bytes")


def test_sanitizer_program_builds_and_exits_0():
    r = subprocess.run(["make", "-C", CSRC, "sanitize_bwd_values_support", "-j4"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    assert "abi_args_bwd_values_support: all argument checks refused as documented" in r.stdout
    assert "runtime error" not in r.stdout + r.stderr and "AddressSanitizer" not in r.stdout + r.stderr


def test_kernel_unit_passes_the_no_scratch_rule():
    """The Makefile's own rule for bwd_values_support.o (cross-compiled for gfx950, no GPU needed; a no-op when the build has
    just made it): 5 kinds x 2 slab widths of nw_bwd_values_support_kernel, no scratch and no spilled vector registers."""
    text = open(os.path.join(CSRC, "Makefile")).read()
    assert "bwd_values_support.hip" in text.split("SRCS :=")[1].split("\n")[0]
    assert "bwd_values_support.o: bwd_values_support.hip" in text and "nw_bwd_values_support_kernelILi" in text
    r = subprocess.run(["make", "-C", CSRC, "bwd_values_support.o"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    remarks = open(os.path.join(CSRC, "bwd_values_support.o.remarks")).read().split("Function Name:")[1:]
    kernels = [k for k in remarks if "nw_bwd_values_support_kernelILi" in k.split("\n")[0]]
    assert len(kernels) == 10
    for k in kernels:
        assert "ScratchSize [bytes/lane]: 0 " in k and "VGPRs Spill: 0 " in k, k.split("\n")[0]


def _aligned(nbytes):
    raw = ctypes.create_string_buffer(nbytes + 16)
    return raw, (ctypes.addressof(raw) + 15) & ~15


def test_workspace_bytes_is_0_outside_the_regime_and_knows_the_modes():
    ws = _lib().load().nw_bwd_values_support_workspace_bytes
    assert ws(8, 1000, 64, 32, 0, 1) > 0 and ws(8, 1000, 64, 16384, 0, 0) > 0 and ws(1, 26, 32, 32, 0, 1) > 0
    # query chunks: partial (N, T) tiles with gvalues, none without; clamped to the 64-query tile count
    assert ws(400, 1000, 64, 64, 3, 1) > ws(400, 1000, 64, 64, 2, 1) > ws(400, 1000, 64, 64, 1, 1) > 0
    assert ws(400, 1000, 64, 64, 1000, 1) == ws(400, 1000, 64, 64, 7, 1)
    assert ws(200, 1000, 64, 64, 1, 1) == ws(200, 1000, 64, 64, 1, 0)          # the whole query loop writes gvalues itself
    N, T = 50000, 512
    assert ws(256, N, 512, T, 0, 0) < N * T * 4 // 4                           # the weights-only mode: nothing of size N x T
    for args in ((0, 1000, 64, 32, 0, 1), (-1, 1000, 64, 32, 0, 1), (8, 25, 64, 32, 0, 1), (8, 1000, 100, 32, 0, 1),
                 (8, 1000, 16, 32, 0, 1), (8, 1000, 64, 0, 0, 1), (8, 1000, 64, 5, 0, 1), (8, 1000, 64, 48, 0, 1),
                 (8, 1000, 64, 16384 + 32, 0, 1), (8, 1000, 64, -32, 0, 1), (8, -1000, 64, 32, 0, 1), (8, 1000, 64, 32, -1, 1)):
        assert ws(*args) == 0, args


def test_refusals_before_any_launch():
    lib = _lib().load()
    B, N, d, T = 8, 1000, 64, 32
    need = lib.nw_bwd_values_support_workspace_bytes(B, N, d, T, 0, 1)
    assert need > 0
    keep, buf = _aligned(256)           # stands for every device pointer: a refused call reads none of them

    def call(q=buf, s=buf, sc=buf, n2=buf, v=buf, a=buf, lo=buf, hi=buf, exclude=0, lse=buf, out=buf, gout=buf, gv=buf, ga=buf,
             ws=buf, ws_bytes=need - 1, B=B, N=N, d=d, T=T, kind=0, chunks=0):
        return lib.nw_bwd_values_support_f32(q, s, sc, n2, v, a, lo, hi, exclude, lse, out, gout, gv, ga, ws, ws_bytes, B, N, d, T,
                                             kind, None, chunks, None)

    assert call(lo=None) == NW_ERR_INVALID_ARG and call(hi=None, exclude=1) == NW_ERR_INVALID_ARG     # half a window
    assert call(gv=None, ga=None) == NW_ERR_INVALID_ARG                          # at least one result
    assert call(a=None) == NW_ERR_INVALID_ARG and call(v=None) == NW_ERR_INVALID_ARG      # glogw needs row_logw and v_rows
    assert call(a=None, v=None, ga=None) == NW_ERR_WORKSPACE                     # ... gvalues alone needs neither
    for mode in (dict(), dict(ga=None, a=None, v=None), dict(gv=None)):          # both, the values alone, the weights alone
        for win in (dict(), dict(lo=None, hi=None)):
            for exclude in (0, 1):
                kw = dict(exclude=exclude, **win, **mode)
                assert call(d=100, **kw) == NW_ERR_UNSUPPORTED                   # nw_fwd_values_f32's regime
                assert call(d=16, **kw) == NW_ERR_UNSUPPORTED
                assert call(N=25, **kw) == NW_ERR_UNSUPPORTED
                for bad_T in (0, 5, 48, 16384 + 32):
                    assert call(T=bad_T, **kw) == NW_ERR_UNSUPPORTED, bad_T
                for name in ("q", "s", "v", "a", "gout", "gv", "ga"):            # 16-byte alignment
                    if kw.get(name, buf) is not None:
                        assert call(**{**kw, name: buf + 4}, ws_bytes=need) == NW_ERR_UNSUPPORTED, name
                assert call(**kw) == NW_ERR_WORKSPACE                            # one byte short
                assert call(ws=None, ws_bytes=need, **kw) == NW_ERR_WORKSPACE
                assert call(ws=buf + 4, ws_bytes=need, **kw) == NW_ERR_UNSUPPORTED
                assert call(B=0, **kw) == NW_OK
                assert call(B=0, q=None, s=None, sc=None, n2=None, lse=None, out=None, gout=None, ws=None, ws_bytes=0,
                            **{**kw, "a": None, "v": None, "gv": None, "ga": None}) == NW_OK
                for name in ("q", "s", "sc", "n2", "lse", "out", "gout"):
                    assert call(**{name: None}, **kw) == NW_ERR_INVALID_ARG, name
                for name in ("B", "N", "d", "T", "chunks"):
                    assert call(**{name: -1}, **kw) == NW_ERR_INVALID_ARG, name
                assert call(kind=4, **kw) == NW_ERR_INVALID_ARG                  # clip without its logit scale
                assert call(kind=7, **kw) == NW_ERR_UNSUPPORTED
    # forced chunks with gvalues: the partial tiles are part of the need
    B2 = 200
    n3 = lib.nw_bwd_values_support_workspace_bytes(B2, N, d, T, 3, 1)
    assert call(B=B2, chunks=3, ws_bytes=n3 - 1) == NW_ERR_WORKSPACE
    del keep


def test_default_path_refusals_are_unchanged():
    from nwhead_amd import ops
    sig = inspect.signature(ops.nw_head_values_bank)
    assert sig.parameters["support_grad"].default is False and list(sig.parameters)[-1] == "support_grad"
    q, s = torch.zeros(4, 64, requires_grad=True), torch.zeros(100, 64)
    for kw in (dict(), dict(support_grad=True)):
        with pytest.raises(ops.NWHipError, match="MI355X"):
            ops.nw_head_values_bank(q, s, None, torch.zeros(100, 3), **kw)          # no CPU path
        with pytest.raises(ops.NWHipError, match="MI355X"):
            ops.nw_head_values_bank(q.detach(), s, None, torch.zeros(100, 3), **kw)
    src = inspect.getsource(ops.nw_head_values_bank)
    # the default's refusal of constants that require grad: the same type, the same text
    assert "differentiates in the queries and a clip scale alone and does not detach silently" in src
    assert "The composition nw_scores + softmax + matmul differentiates in them" in src
    doc = ops.nw_head_values_bank.__doc__
    assert "support_grad=True" in doc and "nw_bwd_values_support_f32" in doc and "BankValues.refresh()" in doc
    assert callable(ops.BankValues.refresh)


def test_nwnet_keywords_exist_and_default_to_todays_behaviour():
    from nwhead_amd.nwhead.nw import NWNet
    assert inspect.signature(NWNet.set_support_values).parameters["learnable"].default is False
    assert inspect.signature(NWNet.forward_values).parameters["weights_grad"].default is False
    assert "support_targets" in NWNet.set_support_values.__doc__ and "weights_grad=True" in NWNet.forward_values.__doc__
