"""The host-side surface of the head's gradient to the bank rows (no GPU): the route rule ops.head_bank_support_route over
plain facts, the declarations and refusals of nw_bwd_bank_support_f32 / nw_bwd_bank_support_workspace_bytes through ctypes,
their stand-alone sanitizer program (tests/sanitize/abi_args_bwd_support.cpp: a host-only AddressSanitizer +
UndefinedBehaviorSanitizer build of the library's own sources against a HIP runtime stand-in; nothing is loaded into
python), the kernel unit's no-scratch rule of the Makefile, and the keywords of ops.nw_head_bank, ops.SplitBank and NWNet."""
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


# ------------------------------------------------------------------------------------------------ the route rule
def test_route_rule_over_plain_facts():
    from nwhead_amd import ops
    ok = dict(split=True, sorted_copy=False, shape=(50000, 512), pad=0, width=512, B=256, n_classes=200)
    route = ops.head_bank_support_route
    for extra in (dict(), dict(window=True), dict(weights=True), dict(window=True, weights=True)):
        assert route(**ok, **extra) == "fused"
    assert route(**{**ok, "shape": (257, 192), "pad": 32, "width": 160}) == "fused"          # a padded bank
    assert route(**{**ok, "shape": (26, 32), "width": 32, "B": 1, "n_classes": 1}) == "fused"  # no size gate
    elsewhere = (dict(split=False), dict(sorted_copy=True), dict(shape=(25, 512)), dict(shape=(50000, 520), width=520),
                 dict(width=500), dict(B=0), dict(n_classes=0))
    for facts in elsewhere:
        f = {**ok, **facts}
        assert route(**f) == "matrix", facts                                                 # nw_head's route computes gs
        why = ops.head_bank_refusal(**f)
        assert why is not None
        for extra, word in ((dict(window=True), "row_window"), (dict(weights=True), "row_logw"),
                            (dict(window=True, weights=True), "row_window")):
            with pytest.raises(ops.NWHipError) as e:
                route(**f, **extra)
            assert "no gradient route" in str(e.value) and why in str(e.value) and word in str(e.value)
    # the same facts, the same answers as the query gradient's rule wherever that one is fused
    assert ops.head_bank_route(**ok) == "fused"


# ------------------------------------------------------------------------------------------------ the C entry
def test_declarations_are_the_headers():
    text = open(os.path.join(ROOT, "include", "nwhead_hip.h")).read()
    assert "int nw_bwd_bank_support_f32(" in text and "size_t nw_bwd_bank_support_workspace_bytes(" in text
    assert "|error of gs[j,k]|" in text                         # the error bound is written down
    decl = text.split("int nw_bwd_bank_support_f32(")[1].split(");")[0]
    sig = _lib().SIGNATURES
    assert len(sig["nw_bwd_bank_support_f32"][1]) == decl.count(",") + 1 == 24
    assert sig["nw_bwd_bank_support_f32"][0] is ctypes.c_int
    wdecl = text.split("size_t nw_bwd_bank_support_workspace_bytes(")[1].split(");")[0]
    assert len(sig["nw_bwd_bank_support_workspace_bytes"][1]) == wdecl.count(",") + 1 == 5
    assert sig["nw_bwd_bank_support_workspace_bytes"][0] is ctypes.c_size_t
    # pointers where the header has pointers, integers where it has integers, in its order
    kinds = [ctypes.c_void_p if "*" in a else (ctypes.c_size_t if "size_t" in a else (ctypes.c_int64 if "int64_t" in a else ctypes.c_int))
             for a in decl.split(",")]
    assert list(sig["nw_bwd_bank_support_f32"][1]) == kinds
    lib = _lib().load()
    assert hasattr(lib, "nw_bwd_bank_support_f32") and hasattr(lib, "nw_bwd_bank_support_workspace_bytes")


def test_sanitizer_program_builds_and_exits_0():
    r = subprocess.run(["make", "-C", CSRC, "sanitize_bwd_support", "-j4"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    assert "abi_args_bwd_support: all argument checks refused as documented" in r.stdout
    assert "runtime error" not in r.stdout + r.stderr and "AddressSanitizer" not in r.stdout + r.stderr


def test_kernel_unit_passes_the_no_scratch_rule():
    """The Makefile's own rule for bwd_support.o (cross-compiled for gfx950, no GPU needed; a no-op when the build has just
    made it): 5 kinds x 2 slab widths of nw_bwd_bank_support_kernel, no scratch and no spilled vector registers."""
    text = open(os.path.join(CSRC, "Makefile")).read()
    assert "bwd_support.hip" in text.split("SRCS :=")[1].split("\n")[0].split()
    assert "bwd_support.o: bwd_support.hip" in text and "nw_bwd_bank_support_kernelILi" in text
    r = subprocess.run(["make", "-C", CSRC, "bwd_support.o"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    remarks = open(os.path.join(CSRC, "bwd_support.o.remarks")).read().split("Function Name:")[1:]
    kernels = [k for k in remarks if "nw_bwd_bank_support_kernelILi" in k.split("\n")[0]]
    assert len(kernels) == 10
    for k in kernels:
        assert "ScratchSize [bytes/lane]: 0 " in k and "VGPRs Spill: 0 " in k, k.split("\n")[0]


def test_workspace_holds_no_score_matrix_and_is_0_outside_the_regime():
    ws = _lib().load().nw_bwd_bank_support_workspace_bytes
    for B, N, d in ((256, 50000, 512), (256, 400000, 256), (256, 32768, 64)):
        assert 0 < ws(B, N, d, 200, 0) < B * N * 4, (B, N, d)
    assert ws(8, 1000, 64, 5, 0) > 0 and ws(1, 26, 32, 1, 0) > 0
    # query chunks: partial (N, d) tiles from the second one on; clamped to the 64-query tile count
    one = ws(400, 1000, 64, 5, 1)
    assert one < 1000 * 64 * 4 and ws(400, 1000, 64, 5, 3) > ws(400, 1000, 64, 5, 2) > one + 2 * 1000 * 64 * 4
    assert ws(400, 1000, 64, 5, 1000) == ws(400, 1000, 64, 5, 7)
    for args in ((0, 1000, 64, 5, 0), (-1, 1000, 64, 5, 0), (8, 0, 64, 5, 0), (8, 25, 64, 5, 0), (8, 1000, 100, 5, 0),
                 (8, 1000, 16, 5, 0), (8, 1000, 0, 5, 0), (8, 1000, 64, 0, 0), (8, 1000, 64, -5, 0), (8, -1000, 64, 5, 0),
                 (8, 1000, 64, 5, -1)):
        assert ws(*args) == 0, args


def _aligned(nbytes):
    raw = ctypes.create_string_buffer(nbytes + 16)
    return raw, (ctypes.addressof(raw) + 15) & ~15


def test_refusals_before_any_launch():
    lib = _lib().load()
    B, N, d, C = 8, 1000, 64, 5
    need = lib.nw_bwd_bank_support_workspace_bytes(B, N, d, C, 0)
    assert need > 0
    keep, buf = _aligned(256)           # stands for every device pointer: a refused call reads none of them

    def call(q=buf, s=buf, sp=buf, sc=buf, n2=buf, sy=buf, a=buf, lo=buf, hi=buf, exclude=0, lse=buf, out=buf, gout=buf, gs=buf,
             ws=buf, ws_bytes=need - 1, B=B, N=N, d=d, C=C, kind=0, chunks=0):
        return lib.nw_bwd_bank_support_f32(q, s, sp, sc, n2, sy, a, lo, hi, exclude, lse, out, gout, gs, ws, ws_bytes, B, N, d, C,
                                           kind, None, chunks, None)

    assert call(lo=None) == NW_ERR_INVALID_ARG and call(hi=None, exclude=1) == NW_ERR_INVALID_ARG     # half a window
    for weights in (dict(), dict(a=None)):
        for win in (dict(), dict(lo=None, hi=None)):
            for exclude in (0, 1):
                kw = dict(exclude=exclude, **win, **weights)
                assert call(d=100, **kw) == NW_ERR_UNSUPPORTED                   # nw_bwd_query_f32's regime
                assert call(d=16, **kw) == NW_ERR_UNSUPPORTED
                assert call(N=25, **kw) == NW_ERR_UNSUPPORTED
                assert call(C=0, **kw) == NW_ERR_UNSUPPORTED
                for name in ("q", "s", "sp", "a", "gs"):                         # 16-byte alignment
                    if kw.get(name, buf) is not None:
                        assert call(**{**kw, name: buf + 4}, ws_bytes=need) == NW_ERR_UNSUPPORTED, name
                assert call(**kw) == NW_ERR_WORKSPACE                            # one byte short
                assert call(ws=None, ws_bytes=need, **kw) == NW_ERR_WORKSPACE
                assert call(ws=buf + 4, ws_bytes=need, **kw) == NW_ERR_UNSUPPORTED
                assert call(B=0, **kw) == NW_OK
                assert call(B=0, q=None, s=None, sp=None, sc=None, n2=None, sy=None, lse=None, out=None, gout=None, gs=None,
                            ws=None, ws_bytes=0, **{**kw, "a": None}) == NW_OK
                for name in ("q", "s", "sp", "sc", "n2", "sy", "lse", "out", "gout", "gs"):
                    assert call(**{name: None}, **kw) == NW_ERR_INVALID_ARG, name
                for name in ("B", "N", "d", "C", "chunks"):
                    assert call(**{name: -1}, **kw) == NW_ERR_INVALID_ARG, name
                assert call(kind=4, **kw) == NW_ERR_INVALID_ARG                  # clip without its logit scale
                assert call(kind=7, **kw) == NW_ERR_UNSUPPORTED
    # forced chunks: the partial tiles are part of the need
    n3 = lib.nw_bwd_bank_support_workspace_bytes(200, N, d, C, 3)
    assert n3 > need and call(B=200, chunks=3, ws_bytes=n3 - 1) == NW_ERR_WORKSPACE
    del keep


# ------------------------------------------------------------------------------------------------ the Python surface
def test_default_path_is_unchanged_and_the_keywords_exist():
    from nwhead_amd import ops
    sig = inspect.signature(ops.nw_head_bank)
    assert sig.parameters["support_grad"].default is False and list(sig.parameters)[-1] == "support_grad"
    src = inspect.getsource(ops.nw_head_bank)
    # the default's refusal of a support that requires grad: the same type, the same text
    assert "nw_head_bank: the bank is a constant here and `s` requires grad; nw_head(q, s, sy, ..., " in src
    assert "support_cache=bank) is the call for support gradients" in src
    q, s = torch.zeros(4, 64, requires_grad=True), torch.zeros(100, 64)
    for kw in (dict(), dict(support_grad=True)):
        with pytest.raises(TypeError, match="prepared bank"):
            ops.nw_head_bank(q, s, torch.zeros(100, dtype=torch.int64), 2, None, **kw)
    doc = ops.nw_head_bank.__doc__
    assert "support_grad=True" in doc and "nw_bwd_bank_support_f32" in doc and "SplitBank.refresh" in doc
    assert callable(ops.SplitBank.refresh) and "class-sorted copy" in ops.SplitBank.refresh.__doc__
    assert list(inspect.signature(ops.head_bank_support_route).parameters) == \
        list(inspect.signature(ops.head_bank_refusal).parameters) + ["window", "weights"]


def test_nwnet_has_the_learnable_bank_and_the_rule_tables_are_as_they_were():
    from nwhead_amd.nwhead import nw
    assert inspect.signature(nw.NWNet.set_bank_learnable).parameters["on"].default is True
    doc = nw.NWNet.set_bank_learnable.__doc__
    assert "support_bank" in doc and "precompute()" in doc and "SplitBank.refresh" in doc
    # bank_rule knows nothing new: learnable rows are no fact of its own
    assert "support_bank" not in inspect.getsource(nw.bank_rule)
    assert "learnable_bank" not in inspect.signature(nw.bank_rule).parameters
