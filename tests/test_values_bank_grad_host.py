"""The host-side surface of the value head's gradient to the bank rows (no GPU): the declarations and refusals of
nw_bwd_values_bank_support_f32 / nw_bwd_values_bank_support_workspace_bytes through ctypes, their stand-alone sanitizer
program (tests/sanitize/abi_args_bwd_values_bank.cpp: a host-only AddressSanitizer + UndefinedBehaviorSanitizer build of the
library's own sources against a HIP runtime stand-in; nothing is loaded into python), the kernel unit's no-scratch rule of the
Makefile, the pure torch support gradient of the matrix route's score node against fp64 autograd of the oracle's scores, and
the keywords of ops.nw_head_values_bank and NWNet.forward_values."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

NW_OK, NW_ERR_INVALID_ARG, NW_ERR_UNSUPPORTED, NW_ERR_WORKSPACE = 0, -1, -2, -3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nwhead_amd", "csrc")
ENTRY, WS = "nw_bwd_values_bank_support_f32", "nw_bwd_values_bank_support_workspace_bytes"
KINDS = ("euclidean", "hypersphere_euclidean", "cosine", "dotproduct", "clip")
LS0 = float(np.log(1 / 0.07))


def _lib():
    from nwhead_amd import _lib
    return _lib


# ------------------------------------------------------------------------------------------------ the C entry
def _ctype(arg):
    return ctypes.c_void_p if "*" in arg else (ctypes.c_size_t if "size_t" in arg else
                                               (ctypes.c_int64 if "int64_t" in arg else ctypes.c_int))


def test_declarations_are_the_headers():
    text = open(os.path.join(ROOT, "include", "nwhead_hip.h")).read()
    assert f"int {ENTRY}(" in text and f"size_t {WS}(" in text
    assert "#define NW_ABI_VERSION 2" in text.replace("  ", " ")
    comment = text.split(f"size_t {WS}(")[0].rsplit("/*", 1)[1]
    for words in ("gs_j = sum_b A_bj q_b + 2 (sum_b r_bj) s_j", "|error of gs[j,k]|", "2.4e-7", "centre such columns", "+0.0",
                  "finite"):
        assert words in comment, words                           # formula, bound, the offset warning, exact zeros, finiteness
    decl = text.split(f"int {ENTRY}(")[1].split(");")[0]
    wdecl = text.split(f"size_t {WS}(")[1].split(");")[0]
    sig = _lib().SIGNATURES
    assert len(sig[ENTRY][1]) == decl.count(",") + 1 == 25 and sig[ENTRY][0] is ctypes.c_int
    assert len(sig[WS][1]) == wdecl.count(",") + 1 == 5 and sig[WS][0] is ctypes.c_size_t
    # pointers where the header has pointers, integers where it has integers, in its order
    assert list(sig[ENTRY][1]) == [_ctype(a) for a in decl.split(",")]
    assert list(sig[WS][1]) == [_ctype(a) for a in wdecl.split(",")]
    # ... and the pair sits where the header has it: behind the class head's gradient to the same rows, in both
    declared = re.findall(r"^(?:int|size_t|int64_t|const char \*)\s*(nw_\w+)\(", text, flags=re.M)
    names = list(sig)
    assert declared.count(ENTRY) == declared.count(WS) == 1
    assert declared[declared.index(WS) - 1:declared.index(WS) + 2] == ["nw_bwd_bank_support_f32", WS, ENTRY]
    assert names[names.index(WS) - 1:names.index(WS) + 2] == ["nw_bwd_bank_support_f32", WS, ENTRY]
    lib = _lib().load()
    assert hasattr(lib, ENTRY) and hasattr(lib, WS)


def test_sanitizer_program_builds_and_exits_0():
    r = subprocess.run(["make", "-C", CSRC, "sanitize_bwd_values_bank", "-j4"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    assert "abi_args_bwd_values_bank: all argument checks refused as documented" in r.stdout
    assert "runtime error" not in r.stdout + r.stderr and "AddressSanitizer" not in r.stdout + r.stderr


def test_kernel_unit_passes_the_no_scratch_rule():
    """The Makefile's own rule for bwd_values_bank.o (cross-compiled for gfx950, no GPU needed; a no-op when the build has just
    made it): 5 kinds x 2 slab widths of nw_bwd_values_bank_support_kernel, no scratch and no spilled vector registers."""
    text = open(os.path.join(CSRC, "Makefile")).read()
    assert "bwd_values_bank.hip" in text.split("SRCS :=")[1].split("\n")[0].split()
    assert "bwd_values_bank.o: bwd_values_bank.hip" in text and "nw_bwd_values_bank_support_kernelILi" in text
    r = subprocess.run(["make", "-C", CSRC, "bwd_values_bank.o"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    remarks = open(os.path.join(CSRC, "bwd_values_bank.o.remarks")).read().split("Function Name:")[1:]
    kernels = [k for k in remarks if "nw_bwd_values_bank_support_kernelILi" in k.split("\n")[0]]
    assert len(kernels) == 10
    for k in kernels:
        assert "ScratchSize [bytes/lane]: 0 " in k and "VGPRs Spill: 0 " in k, k.split("\n")[0]
    # the finish kernel and the layout pieces are the skeleton's, written once
    core = open(os.path.join(CSRC, "bwd_support_core.h")).read()
    assert "nw_bwd_support_rows_finish_kernel" in core and "sup_rows_layout" in core
    for unit in ("bwd_support.hip", "bwd_values_bank.hip"):
        src = open(os.path.join(CSRC, unit)).read()
        assert "launch_sup_rows_finish(" in src and "sup_rows_layout(" in src and "finish_kernel(" not in src, unit


def test_workspace_holds_no_score_matrix_and_is_0_outside_the_regime():
    ws = getattr(_lib().load(), WS)
    for B, N, d in ((256, 50000, 512), (256, 400000, 256)):                      # the two bank shapes
        for T in (32, 512):
            assert 0 < ws(B, N, d, T, 0) < B * N * 4, (B, N, d, T)
    assert ws(8, 1000, 64, 32, 0) > 0 and ws(1, 26, 32, 32, 0) > 0
    assert ws(256, 50000, 512, 32, 0) == ws(256, 50000, 512, 16384, 0)           # nothing of size N x T: T does not enter
    # query chunks: partial (N, d) tiles from the second one on; clamped to the 64-query tile count
    one = ws(400, 1000, 64, 32, 1)
    assert one < 1000 * 64 * 4 and ws(400, 1000, 64, 32, 3) > ws(400, 1000, 64, 32, 2) > one + 2 * 1000 * 64 * 4
    assert ws(400, 1000, 64, 32, 1000) == ws(400, 1000, 64, 32, 7)
    for args in ((0, 1000, 64, 32, 0), (-1, 1000, 64, 32, 0), (8, 0, 64, 32, 0), (8, 25, 64, 32, 0), (8, 1000, 100, 32, 0),
                 (8, 1000, 16, 32, 0), (8, 1000, 0, 32, 0), (8, 1000, 64, 0, 0), (8, 1000, 64, 5, 0), (8, 1000, 64, 48, 0),
                 (8, 1000, 64, 16384 + 32, 0), (8, 1000, 64, -32, 0), (8, -1000, 64, 32, 0), (8, 1000, 64, 32, -1)):
        assert ws(*args) == 0, args


def _aligned(nbytes):
    raw = ctypes.create_string_buffer(nbytes + 16)
    return raw, (ctypes.addressof(raw) + 15) & ~15


def test_refusals_before_any_launch():
    lib = _lib().load()
    fn, wsf = getattr(lib, ENTRY), getattr(lib, WS)
    B, N, d, T = 8, 1000, 64, 32
    need = wsf(B, N, d, T, 0)
    assert need > 0
    keep, buf = _aligned(256)           # stands for every device pointer: a refused call reads none of them

    def call(q=buf, s=buf, sp=buf, sc=buf, n2=buf, vp=buf, vs=buf, a=buf, lo=buf, hi=buf, exclude=0, lse=buf, out=buf, gout=buf,
             gs=buf, ws=buf, ws_bytes=need - 1, B=B, N=N, d=d, T=T, kind=0, chunks=0):
        return fn(q, s, sp, sc, n2, vp, vs, a, lo, hi, exclude, lse, out, gout, gs, ws, ws_bytes, B, N, d, T, kind, None, chunks, None)

    assert call(lo=None) == NW_ERR_INVALID_ARG and call(hi=None, exclude=1) == NW_ERR_INVALID_ARG     # half a window
    for weights in (dict(), dict(a=None)):
        for win in (dict(), dict(lo=None, hi=None)):
            for exclude in (0, 1):
                kw = dict(exclude=exclude, **win, **weights)
                assert call(d=100, **kw) == NW_ERR_UNSUPPORTED                   # nw_fwd_values_f32's regime
                assert call(d=16, **kw) == NW_ERR_UNSUPPORTED
                assert call(N=25, **kw) == NW_ERR_UNSUPPORTED
                for bad_T in (0, 5, 48, 16384 + 32):
                    assert call(T=bad_T, **kw) == NW_ERR_UNSUPPORTED, bad_T
                for name in ("q", "s", "sp", "vp", "a", "gout", "gs"):           # 16-byte alignment
                    if kw.get(name, buf) is not None:
                        assert call(**{**kw, name: buf + 4}, ws_bytes=need) == NW_ERR_UNSUPPORTED, name
                assert call(**kw) == NW_ERR_WORKSPACE                            # one byte short
                assert call(ws=None, ws_bytes=need, **kw) == NW_ERR_WORKSPACE
                assert call(ws=buf + 4, ws_bytes=need, **kw) == NW_ERR_UNSUPPORTED
                assert call(B=0, **kw) == NW_OK
                assert call(B=0, q=None, s=None, sp=None, sc=None, n2=None, vp=None, vs=None, lse=None, out=None, gout=None,
                            gs=None, ws=None, ws_bytes=0, **{**kw, "a": None}) == NW_OK
                for name in ("q", "s", "sp", "sc", "n2", "vp", "vs", "lse", "out", "gout", "gs"):
                    assert call(**{name: None}, **kw) == NW_ERR_INVALID_ARG, name
                for name in ("B", "N", "d", "T", "chunks"):
                    assert call(**{name: -1}, **kw) == NW_ERR_INVALID_ARG, name
                # the order of the checks: a negative size before the kind, the kind before the regime, the regime before
                # the pointers, the pointers before the alignment, the alignment before the workspace
                assert call(B=-1, kind=7, **kw) == NW_ERR_INVALID_ARG
                assert call(kind=7, q=None, **kw) == NW_ERR_UNSUPPORTED
                assert call(d=100, q=None, **kw) == NW_ERR_UNSUPPORTED
                assert call(q=None, gs=buf + 4, **kw) == NW_ERR_INVALID_ARG
                assert call(gs=buf + 4, **kw) == NW_ERR_UNSUPPORTED
                assert call(kind=4, **kw) == NW_ERR_INVALID_ARG                  # clip without its logit scale
                assert call(kind=7, **kw) == NW_ERR_UNSUPPORTED
    # forced chunks: the partial tiles are part of the need
    n3 = wsf(200, N, d, T, 3)
    assert n3 > need and call(B=200, chunks=3, ws_bytes=n3 - 1) == NW_ERR_WORKSPACE
    del keep


# ------------------------------------------------------------------------------------------------ the matrix route's score node
def _scores_with_convention(O, q, s, kind):
    """The oracle's fp64 scores; for the distance kinds its values with no gradient at a distance of exactly 0 (head_f64 of
    test_bank_support_grad_gpu.py)."""
    if kind in ("euclidean", "hypersphere_euclidean"):
        xq, sx = q[:, None, :], s[None]
        if kind == "hypersphere_euclidean":
            xq = xq / xq.norm(dim=-1, keepdim=True).clamp_min(1e-12)
            sx = sx / sx.norm(dim=-1, keepdim=True).clamp_min(1e-12)
        d2 = (xq - sx).pow(2).sum(-1)
        sc = -torch.where(d2 > 0, torch.where(d2 > 0, d2, torch.ones_like(d2)).sqrt(), torch.zeros_like(d2))
        assert torch.equal(sc.detach(), O.scores_f64(q.detach(), s.detach(), kind, LS0))
        return sc
    return O.scores_f64(q, s, kind, LS0)


@pytest.mark.parametrize("kind", KINDS)
def test_support_gradient_of_the_score_node_matches_fp64_autograd_of_the_oracle(kind):
    from nwhead_amd import ops
    from oracle import nw_oracle as O
    g = torch.Generator().manual_seed(3)
    B, N, d = 9, 14, 8
    q, s = torch.randn(B, d, generator=g, dtype=torch.float64), torch.randn(N, d, generator=g, dtype=torch.float64)
    s[4] = 0.0                                                   # a zero row (the clamp of the normalising kinds)
    q[2] = s[7]                                                  # a coincident pair: distance exactly 0
    gsc = torch.randn(B, N, generator=g, dtype=torch.float64)
    sl = s.clone().requires_grad_(True)
    sc = _scores_with_convention(O, q, sl, kind)
    ref = torch.autograd.grad((sc * gsc).sum(), sl)[0]
    scale = torch.tensor(LS0, dtype=torch.float64).exp() if kind == "clip" else None
    got = ops._scores_support_grad(q, s, sc.detach(), gsc, ops.SCORE_KINDS[kind], scale)
    assert got.shape == (N, d) and got.dtype == torch.float64
    norm = max(float(ref.abs().max()), 1e-3)
    err = float((got - ref).abs().max()) / norm
    print(f"ERR {err:.3e} _scores_support_grad {kind}")
    assert err < 1e-10, (kind, err)                              # fp64 against fp64: rounding alone
    assert bool((got[4] == 0).all()) == bool((ref[4] == 0).all())
    # the node computes it only when `s` needs it
    src = inspect.getsource(ops._ScoresFn.backward)
    assert "_scores_support_grad(" in src and "needs_input_grad[2]" in src


# ------------------------------------------------------------------------------------------------ the Python surface
def test_keywords_docstrings_and_the_default_refusal():
    from nwhead_amd import ops
    from nwhead_amd.nwhead import nw
    sig = inspect.signature(ops.nw_head_values_bank)
    assert sig.parameters["support_grad"].default is False and list(sig.parameters)[-1] == "support_grad"
    src = inspect.getsource(ops.nw_head_values_bank)
    # the default's refusal of a support that requires grad: the same type, the same text
    assert 'raise ValueError("nw_head_values_bank: the bank is a constant here and `s` requires grad")' in src
    assert "grad_s = bool(support_grad and grad and s.requires_grad)" in src
    doc = ops.nw_head_values_bank.__doc__
    for words in ("LEARNABLE BANK ROWS", ENTRY, "SplitBank.refresh", "4.8n"):
        assert words in doc, words
    assert ENTRY in inspect.getsource(ops._values_bank_support_bwd)
    node = inspect.getsource(ops._NWValuesBankFn)
    assert "_values_bank_support_bwd(" in node and "bank.rows if bank.rows is not None" in node
    assert list(inspect.signature(ops.head_values_grad_route).parameters) == list(inspect.signature(ops.head_values_route).parameters)
    fv = nw.NWNet.forward_values
    assert "support_bank" in fv.__doc__ and "set_bank_learnable()" in fv.__doc__ and "4.8n" in fv.__doc__
    assert "support_bank" in inspect.getsource(fv) and '"support_grad": True' in inspect.getsource(fv)
    assert "forward_values" in nw.NWNet.set_bank_learnable.__doc__
    # bank_rule knows nothing new: learnable rows are no fact of its own
    assert "support_bank" not in inspect.getsource(nw.bank_rule)
    assert "learnable_bank" not in inspect.signature(nw.bank_rule).parameters
