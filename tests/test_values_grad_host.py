"""The host-side surface of the value head's query gradient (no GPU): the declarations and refusals of
nw_bwd_values_query_f32 / nw_bwd_values_query_workspace_bytes through ctypes, their stand-alone sanitizer program
(tests/sanitize/abi_args_bwd_values.cpp: a host-only AddressSanitizer + UndefinedBehaviorSanitizer build of the library's own
sources against a HIP runtime stand-in; nothing is loaded into python), the kernel unit's no-scratch rule of the Makefile, the
route rule as a pure function, nw.bank_rule's answers for forward_values, and what NWNet.forward_values and
ops.nw_head_values_bank refuse before any device work."""
import ctypes
import os
import subprocess

import pytest
import torch
import torch.nn as nn

NW_OK, NW_ERR_INVALID_ARG, NW_ERR_UNSUPPORTED, NW_ERR_WORKSPACE = 0, -1, -2, -3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nwhead_amd", "csrc")


def _lib():
    from nwhead_amd import _lib
    return _lib


def test_declarations_are_the_headers():
    text = open(os.path.join(ROOT, "include", "nwhead_hip.h")).read()
    assert "int nw_bwd_values_query_f32(" in text and "size_t nw_bwd_values_query_workspace_bytes(" in text
    assert "#define NW_ABI_VERSION 2" in text.replace("  ", " ")
    assert "centre such columns" in text                    # the accuracy limit of c - m is written down
    sig = _lib().SIGNATURES
    assert len(sig["nw_bwd_values_query_f32"][1]) == 25 and len(sig["nw_bwd_values_query_workspace_bytes"][1]) == 5
    assert sig["nw_bwd_values_query_workspace_bytes"][0] is ctypes.c_size_t
    lib = _lib().load()
    assert hasattr(lib, "nw_bwd_values_query_f32") and hasattr(lib, "nw_bwd_values_query_workspace_bytes")


def test_sanitizer_program_builds_and_exits_0():
    r = subprocess.run(["make", "-C", CSRC, "sanitize_bwd_values", "-j4"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    assert "abi_args_bwd_values: all argument checks refused as documented" in r.stdout
    assert "runtime error" not in r.stdout + r.stderr and "AddressSanitizer" not in r.stdout + r.stderr


def test_kernel_unit_passes_the_no_scratch_rule():
    """The Makefile's own rule for bwd_values.o (cross-compiled for gfx950, no GPU needed; a no-op when the build has just
    made it): 5 kinds x 2 slab widths of nw_bwd_values_query_kernel, no scratch and no spilled vector registers -- read once
    more from the remarks the rule leaves."""
    text = open(os.path.join(CSRC, "Makefile")).read()
    assert "bwd_values.hip" in text.split("SRCS :=")[1].split("\n")[0]
    assert "bwd_values.o: bwd_values.hip" in text and "nw_bwd_values_query_kernelILi" in text
    r = subprocess.run(["make", "-C", CSRC, "bwd_values.o"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    remarks = open(os.path.join(CSRC, "bwd_values.o.remarks")).read().split("Function Name:")[1:]
    kernels = [k for k in remarks if "nw_bwd_values_query_kernelILi" in k.split("\n")[0]]
    assert len(kernels) == 10
    for k in kernels:
        assert "ScratchSize [bytes/lane]: 0 " in k and "VGPRs Spill: 0 " in k, k.split("\n")[0]


def _aligned(nbytes):
    raw = ctypes.create_string_buffer(nbytes + 16)
    return raw, (ctypes.addressof(raw) + 15) & ~15


def test_workspace_bytes_is_0_outside_the_regime_and_grows_with_chunks():
    ws = _lib().load().nw_bwd_values_query_workspace_bytes
    assert ws(8, 1000, 64, 32, 0) > 0 and ws(8, 1000, 64, 16384, 0) > 0 and ws(1, 26, 32, 32, 0) > 0
    assert ws(8, 1000, 64, 64, 3) > ws(8, 1000, 64, 64, 2) > ws(8, 1000, 64, 64, 1) > 0    # the chunks' partial tiles
    assert ws(8, 1000, 64, 64, 1000) == ws(8, 1000, 64, 64, 16)             # ... clamped to the 64-row tile count
    assert ws(8, 1000, 64, 32, 1) == ws(8, 1000, 64, 512, 1)                # partial tiles of gq: (B, d), whatever T
    for args in ((0, 1000, 64, 32, 0), (-1, 1000, 64, 32, 0), (8, 25, 64, 32, 0), (8, 1000, 100, 32, 0), (8, 1000, 16, 32, 0),
                 (8, 1000, 64, 0, 0), (8, 1000, 64, 5, 0), (8, 1000, 64, 48, 0), (8, 1000, 64, 16384 + 32, 0),
                 (8, 1000, 64, -32, 0), (8, -1000, 64, 32, 0), (8, 1000, 64, 32, -1)):
        assert ws(*args) == 0, args


def test_refusals_before_any_launch():
    lib = _lib().load()
    B, N, d, T = 8, 1000, 64, 32
    need = lib.nw_bwd_values_query_workspace_bytes(B, N, d, T, 0)
    assert need > 0
    keep, buf = _aligned(256)           # stands for every device pointer: a refused call reads none of them

    def call(q=buf, s=buf, sc=buf, n2=buf, v=buf, vs=buf, a=buf, lo=buf, hi=buf, exclude=0, lse=buf, out=buf, gout=buf, gq=buf,
             gls=buf, ws=buf, ws_bytes=need - 1, B=B, N=N, d=d, T=T, kind=0, chunks=0):
        return lib.nw_bwd_values_query_f32(q, s, sc, n2, v, vs, a, lo, hi, exclude, lse, out, gout, gq, gls, ws, ws_bytes, B, N, d,
                                           T, kind, None, chunks, None)

    assert call(lo=None) == NW_ERR_INVALID_ARG and call(hi=None, exclude=1) == NW_ERR_INVALID_ARG     # half a window
    for weights in (dict(), dict(a=None)):                                       # the weights are optional
        for win in (dict(), dict(lo=None, hi=None)):                             # with a window and without
            for exclude in (0, 1):
                kw = dict(exclude=exclude, **win, **weights)
                assert call(d=100, **kw) == NW_ERR_UNSUPPORTED                   # nw_fwd_values_f32's regime
                assert call(d=16, **kw) == NW_ERR_UNSUPPORTED
                assert call(N=25, **kw) == NW_ERR_UNSUPPORTED
                for bad_T in (0, 5, 48, 16384 + 32):                             # T: a multiple of 32 in [32, 16384]
                    assert call(T=bad_T, **kw) == NW_ERR_UNSUPPORTED, bad_T
                for name in ("q", "s", "v", "gout", "gq"):                       # 16-byte alignment
                    assert call(**{name: buf + 4}, ws_bytes=need, **kw) == NW_ERR_UNSUPPORTED, name
                if "a" not in weights:
                    assert call(ws_bytes=need, **{**kw, "a": buf + 4}) == NW_ERR_UNSUPPORTED      # float4 reads of the weights
                assert call(**kw) == NW_ERR_WORKSPACE                            # one byte short
                assert call(ws=None, ws_bytes=need, **kw) == NW_ERR_WORKSPACE
                assert call(ws=buf + 4, ws_bytes=need, **kw) == NW_ERR_UNSUPPORTED
                assert call(chunks=3, ws_bytes=lib.nw_bwd_values_query_workspace_bytes(B, N, d, T, 3) - 1, **kw) == NW_ERR_WORKSPACE
                assert call(B=0, **kw) == NW_OK
                assert call(B=0, q=None, s=None, sc=None, n2=None, v=None, vs=None, lse=None, out=None, gout=None, gq=None, gls=None,
                            ws=None, ws_bytes=0, **{**kw, "a": None}) == NW_OK
                for name in ("q", "s", "sc", "n2", "v", "vs", "lse", "out", "gout", "gq"):
                    assert call(**{name: None}, **kw) == NW_ERR_INVALID_ARG, name
                for name in ("B", "N", "d", "T", "chunks"):
                    assert call(**{name: -1}, **kw) == NW_ERR_INVALID_ARG, name
                assert call(kind=4, **kw) == NW_ERR_INVALID_ARG                  # clip without its logit scale
                assert call(kind=7, **kw) == NW_ERR_UNSUPPORTED
    del keep


def test_grad_route_rule():
    from nwhead_amd.ops import HEAD_VALUES_MAX_T, head_values_grad_route, head_values_route
    base = dict(split=True, sorted_copy=False, shape=(50000, 512), pad=0, width=512, B=256)
    table = [
        (base, 32, "fused"), (base, 1, "fused"), (base, 5, "fused"), (base, HEAD_VALUES_MAX_T, "fused"),
        (base, HEAD_VALUES_MAX_T + 1, "matrix"), (base, 0, "matrix"),
        ({**base, "shape": (26, 32), "width": 32, "B": 1}, 1, "fused"),
        ({**base, "pad": 12, "width": 500}, 40, "fused"),                        # queries that pad to the bank
        ({**base, "split": False}, 32, "matrix"),                                # an fp16 or norms-only bank
        ({**base, "sorted_copy": True}, 32, "matrix"),                           # a class-sorted copy
        ({**base, "shape": (25, 512)}, 32, "matrix"),                            # N <= 25
        ({**base, "shape": (20, 512)}, 32, "matrix"),
        ({**base, "width": 500}, 32, "matrix"),                                  # widths that do not pad
        ({**base, "shape": (50000, 500), "width": 500}, 32, "matrix"),
        ({**base, "B": 0}, 32, "matrix"),
    ]
    for facts, T, want in table:
        assert head_values_grad_route(**facts, T=T) == want, (facts, T)
        assert head_values_grad_route(**facts, T=T) == head_values_route(**facts, T=T)    # fused exactly where the forward is


def test_bank_rule_forward_values_and_old_answers():
    from nwhead_amd.nwhead.nw import WHAT, Refusal, bank_rule
    from nwhead_amd.ops import NWHipError
    assert WHAT["forward_values"] == "forward_values"
    for kw in (dict(resident=True, sharded=False), dict(resident=False, sharded=False), dict(resident=False, sharded=True),
               dict(resident=True, sharded=True), dict(resident=True, sharded=False, builtin_kernel=False),
               dict(resident=True, sharded=False, weights="constant"), dict(resident=True, sharded=False, weights="learnable")):
        got, twin = bank_rule("forward_values", **kw), bank_rule("predict_values", **kw)
        if isinstance(twin, Refusal):       # the same answer as predict_values, under its own name
            assert isinstance(got, Refusal) and (got.kind, got.early) == (twin.kind, twin.early)
            assert got.text == twin.text.replace("predict_values", "forward_values") and "forward_values" in got.text
        else:
            assert got == twin == "resident"
    r = bank_rule("forward_values", resident=False, sharded=False)
    assert r.kind is NWHipError and r.early and "precompute()" in r.text
    assert "sharded" in bank_rule("forward_values", resident=True, sharded=True).text
    assert not bank_rule("forward_values", resident=True, sharded=False, builtin_kernel=False).early
    # every previous entry answers what it did
    for entry in ("set_support_values", "predict_values", "predict_loo_values", "forward_bank", "refresh_bank", "predict_loo"):
        assert WHAT[entry] == entry
        assert bank_rule(entry, resident=True, sharded=False) == "resident"
        assert isinstance(bank_rule(entry, resident=False, sharded=False), Refusal)
    assert bank_rule("set_support_values", resident=True, sharded=True) == "resident"
    assert bank_rule("set_support_weights", resident=True, sharded=True) == "resident"
    assert "the weights are rows" in bank_rule("set_support_weights", resident=False, sharded=True).text
    for entry in ("predict_values", "predict_loo_values", "predict_loo", "forward_bank"):
        assert isinstance(bank_rule(entry, resident=True, sharded=True), Refusal)
    assert bank_rule("predict", resident=True, sharded=True, searchable=True, mode="full") == "sharded"
    assert bank_rule("predict", resident=True, sharded=False, searchable=True, mode="full") == "resident"
    assert bank_rule("predict", resident=True, sharded=False, searchable=True, mode="knn") == "supports"
    assert bank_rule("get_neighbors", resident=False, sharded=True, k_given=True) == "sharded"
    assert isinstance(bank_rule("get_neighbors", resident=False, sharded=True, k_given=False), Refusal)
    assert bank_rule("explain", resident=True, sharded=True) == "resident"
    assert bank_rule("weights_for", "forward_bank", resident=True, sharded=False, weights="constant") == "resident"


class _DS(torch.utils.data.Dataset):
    def __init__(self, data, targets, C):
        self.data, self.targets, self.num_classes = data, list(targets), C

    def __len__(self):
        return len(self.targets)

    def __getitem__(self, i):
        return self.data[i], self.targets[i]


class _Counting(nn.Linear):
    calls = 0

    def forward(self, x):
        type(self).calls += 1
        return super().forward(x)


def test_nwnet_forward_values_refuses_a_missing_bank_and_missing_values():
    from nwhead_amd.nwhead.nw import NWNet
    from nwhead_amd.ops import NWHipError
    g = torch.Generator().manual_seed(5)
    ds = _DS(torch.randn(24, 8, generator=g), [i % 4 for i in range(24)], 4)
    feat = _Counting(8, 32)
    net = NWNet(feat, 4, support_dataset=ds, n_shot=2, n_way=4, n_shot_full=6, device="cpu")
    n0 = _Counting.calls
    with pytest.raises(NWHipError, match="forward_values needs the bank of precompute"):
        net.forward_values(torch.zeros(2, 8))
    # a resident bank without values: refused by name, before the featurizer runs
    net.full_feat, net.full_y = torch.randn(24, 32, generator=g), torch.arange(24) % 4
    assert net.support_values is None
    with pytest.raises(NWHipError, match="forward_values: no values are set.*set_support_values"):
        net.forward_values(torch.zeros(2, 8))
    assert _Counting.calls == n0
    doc = NWNet.forward_values.__doc__
    assert "Not in the reference" in doc and "read detached" in doc and "centre" in doc


def test_nwnet_forward_values_refuses_a_sharded_bank():
    from test_sharded_knn_host import _net
    from nwhead_amd.ops import NWHipError
    net = _net()
    hook = lambda *a: None  # noqa: E731  (the compute hooks of the CPU tests: nothing is computed here)
    with torch.no_grad():
        net.precompute_sharded(partial_fn=hook, merge_fn=hook, search_fn=hook, knn_merge_fn=hook)
    with pytest.raises(NWHipError, match="forward_values: a sharded bank"):
        net.forward_values(torch.zeros(2, 8))


def test_nw_head_values_bank_refuses_on_the_host():
    from nwhead_amd import ops
    q, s = torch.zeros(4, 64, requires_grad=True), torch.zeros(100, 64)
    with pytest.raises(ops.NWHipError, match="MI355X"):
        ops.nw_head_values_bank(q, s, None, torch.zeros(100, 3))          # no CPU path
    with pytest.raises(ops.NWHipError, match="MI355X"):
        ops.nw_head_values_bank(q.detach(), s, None, torch.zeros(100, 3))
    assert "centre" in ops.nw_head_values_bank.__doc__.lower() and "nw_bwd_values_query_f32" in ops.nw_head_values_bank.__doc__
