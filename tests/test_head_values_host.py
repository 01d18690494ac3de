"""The host-side surface of the value head (no GPU): the declarations and refusals of nw_fwd_values_f32 /
nw_fwd_values_workspace_bytes through ctypes, their stand-alone sanitizer program (tests/sanitize/abi_args_fwd_values.cpp: a
host-only AddressSanitizer + UndefinedBehaviorSanitizer build of the library's own sources against a HIP runtime stand-in;
nothing is loaded into python), the route rule as a pure function, nw.bank_rule's answers for the new entry points, and what
NWNet refuses before any device work."""
import ctypes
import os
import subprocess

import pytest
import torch
import torch.nn as nn

NW_OK, NW_ERR_INVALID_ARG, NW_ERR_UNSUPPORTED, NW_ERR_WORKSPACE = 0, -1, -2, -3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from nwhead_amd import _lib
    return _lib


def test_declarations_are_the_headers():
    text = open(os.path.join(ROOT, "include", "nwhead_hip.h")).read()
    assert "int nw_fwd_values_f32(" in text and "size_t nw_fwd_values_workspace_bytes(" in text
    assert "#define NW_ABI_VERSION 2" in text.replace("  ", " ")
    assert "0 x inf is NaN" in text                      # the finite-values contract is written down
    sig = _lib().SIGNATURES
    assert len(sig["nw_fwd_values_f32"][1]) == 22 and len(sig["nw_fwd_values_workspace_bytes"][1]) == 5
    assert sig["nw_fwd_values_workspace_bytes"][0] is ctypes.c_size_t


def test_sanitizer_program_builds_and_exits_0():
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "nwhead_amd", "csrc"), "sanitize_fwd_values", "-j4"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    assert "abi_args_fwd_values: all argument checks refused as documented" in r.stdout
    assert "runtime error" not in r.stdout + r.stderr and "AddressSanitizer" not in r.stdout + r.stderr


def _aligned(nbytes):
    raw = ctypes.create_string_buffer(nbytes + 16)
    return raw, (ctypes.addressof(raw) + 15) & ~15


def test_workspace_bytes_is_0_outside_the_regime():
    ws = _lib().load().nw_fwd_values_workspace_bytes
    assert ws(8, 1000, 64, 32, 0) > 0 and ws(8, 1000, 64, 16384, 0) > 0 and ws(1, 26, 32, 32, 0) > 0
    assert ws(8, 1000, 64, 64, 3) > ws(8, 1000, 64, 64, 1) > 0              # a forced chunk count sizes the partial tiles
    assert ws(8, 1000, 64, 64, 1000) == ws(8, 1000, 64, 64, 16)             # ... clamped to the 64-row tile count
    for args in ((0, 1000, 64, 32, 0), (-1, 1000, 64, 32, 0), (8, 25, 64, 32, 0), (8, 1000, 100, 32, 0), (8, 1000, 16, 32, 0),
                 (8, 1000, 64, 0, 0), (8, 1000, 64, 5, 0), (8, 1000, 64, 48, 0), (8, 1000, 64, 16384 + 32, 0),
                 (8, 1000, 64, -32, 0), (8, -1000, 64, 32, 0), (8, 1000, 64, 32, -1)):
        assert ws(*args) == 0, args


def test_refusals_before_any_launch():
    lib = _lib().load()
    B, N, d, T = 8, 1000, 64, 32
    need = lib.nw_fwd_values_workspace_bytes(B, N, d, T, 0)
    assert need > 0
    keep, buf = _aligned(256)           # stands for every device pointer: a refused call reads none of them

    def call(q=buf, s=buf, sc=buf, n2=buf, v=buf, vs=buf, a=buf, lo=buf, hi=buf, exclude=0, lse=buf, out=buf, ws=buf,
             ws_bytes=need - 1, B=B, N=N, d=d, T=T, kind=0, chunks=0):
        return lib.nw_fwd_values_f32(q, s, sc, n2, v, vs, a, lo, hi, exclude, lse, out, ws, ws_bytes, B, N, d, T, kind, None,
                                     chunks, None)

    assert call(lo=None) == NW_ERR_INVALID_ARG and call(hi=None, exclude=1) == NW_ERR_INVALID_ARG     # half a window
    for weights in (dict(), dict(a=None)):                                       # the weights are optional
        for win in (dict(), dict(lo=None, hi=None)):                             # with a window and without
            for exclude in (0, 1):
                kw = dict(exclude=exclude, **win, **weights)
                assert call(d=100, **kw) == NW_ERR_UNSUPPORTED                   # nw_fwd_window_f32's regime
                assert call(d=16, **kw) == NW_ERR_UNSUPPORTED
                assert call(N=25, **kw) == NW_ERR_UNSUPPORTED
                for bad_T in (0, 5, 48, 16384 + 32):                             # T: a multiple of 32 in [32, 16384]
                    assert call(T=bad_T, **kw) == NW_ERR_UNSUPPORTED, bad_T
                for name in ("q", "s", "v", "out"):                              # 16-byte alignment
                    assert call(**{name: buf + 4}, ws_bytes=need, **kw) == NW_ERR_UNSUPPORTED, name
                if "a" not in weights:
                    assert call(ws_bytes=need, **{**kw, "a": buf + 4}) == NW_ERR_UNSUPPORTED      # float4 reads of the weights
                assert call(**kw) == NW_ERR_WORKSPACE                            # one byte short
                assert call(ws=None, ws_bytes=need, **kw) == NW_ERR_WORKSPACE
                assert call(ws=buf + 4, ws_bytes=need, **kw) == NW_ERR_UNSUPPORTED
                assert call(chunks=3, ws_bytes=lib.nw_fwd_values_workspace_bytes(B, N, d, T, 3) - 1, **kw) == NW_ERR_WORKSPACE
                assert call(B=0, **kw) == NW_OK
                assert call(B=0, q=None, s=None, sc=None, n2=None, v=None, vs=None, lse=None, out=None, ws=None, ws_bytes=0,
                            **{**kw, "a": None}) == NW_OK
                for name in ("q", "s", "sc", "n2", "v", "vs", "lse", "out"):
                    assert call(**{name: None}, **kw) == NW_ERR_INVALID_ARG, name
                for name in ("B", "N", "d", "T", "chunks"):
                    assert call(**{name: -1}, **kw) == NW_ERR_INVALID_ARG, name
                assert call(kind=4, **kw) == NW_ERR_INVALID_ARG                  # clip without its logit scale
                assert call(kind=7, **kw) == NW_ERR_UNSUPPORTED
    del keep


def test_route_rule():
    from nwhead_amd.ops import HEAD_VALUES_MAX_T, head_values_route, head_window_route
    base = dict(split=True, sorted_copy=False, shape=(50000, 512), pad=0, width=512, B=256)
    table = [
        (base, 32, "fused"), (base, 1, "fused"), (base, 5, "fused"), (base, HEAD_VALUES_MAX_T, "fused"),
        (base, HEAD_VALUES_MAX_T + 1, "matrix"), (base, 0, "matrix"),
        ({**base, "shape": (26, 32), "width": 32, "B": 1}, 1, "fused"),
        ({**base, "pad": 12, "width": 500}, 40, "fused"),                        # queries that pad to the bank
        ({**base, "split": False}, 32, "matrix"),                                # an fp16 or norms-only bank
        ({**base, "sorted_copy": True}, 32, "matrix"),                           # a class-sorted copy
        ({**base, "shape": (25, 512)}, 32, "matrix"),                            # N <= 25
        ({**base, "width": 500}, 32, "matrix"),                                  # widths that do not pad
        ({**base, "shape": (50000, 500), "width": 500}, 32, "matrix"),
        ({**base, "B": 0}, 32, "matrix"),
    ]
    assert HEAD_VALUES_MAX_T == 16384
    for facts, T, want in table:
        assert head_values_route(**facts, T=T) == want, (facts, T)
        if 1 <= T <= HEAD_VALUES_MAX_T:       # fused exactly where the windowed head of one class is
            assert head_values_route(**facts, T=T) == head_window_route(**facts, n_classes=1)


def test_bank_rule_new_entries_and_old_answers():
    from nwhead_amd.nwhead.nw import WHAT, Refusal, bank_rule
    from nwhead_amd.ops import NWHipError
    for entry in ("set_support_values", "predict_values", "predict_loo_values"):
        assert WHAT[entry] == entry
        assert bank_rule(entry, resident=True, sharded=False) == "resident"
        r = bank_rule(entry, resident=False, sharded=False)
        assert isinstance(r, Refusal) and r.kind is NWHipError and r.early and "precompute()" in r.text and entry in r.text
        r = bank_rule(entry, resident=False, sharded=True)
        assert isinstance(r, Refusal) and r.kind is NWHipError and r.early and "sharded" in r.text
        r = bank_rule(entry, resident=True, sharded=False, builtin_kernel=False)
        assert isinstance(r, Refusal) and not r.early and "built-in score kernels" in r.text
    # the values are rows of ONE resident bank: a resident bank beside a sharded one takes them, like the weights; the value
    # head over a row window does not look past the sharded bank, like predict_loo
    assert bank_rule("set_support_values", resident=True, sharded=True) == "resident"
    assert "the values are rows" in bank_rule("set_support_values", resident=False, sharded=True).text
    for entry in ("predict_values", "predict_loo_values"):
        assert isinstance(bank_rule(entry, resident=True, sharded=True), Refusal)
    # the old entries answer what they did
    assert bank_rule("set_support_weights", resident=True, sharded=True) == "resident"
    assert "the weights are rows" in bank_rule("set_support_weights", resident=False, sharded=True).text
    assert bank_rule("predict_loo", resident=True, sharded=False) == "resident"
    assert isinstance(bank_rule("predict_loo", resident=True, sharded=True), Refusal)
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


def test_nwnet_refuses_without_a_bank():
    from nwhead_amd.nwhead.nw import NWNet
    from nwhead_amd.ops import NWHipError
    g = torch.Generator().manual_seed(5)
    ds = _DS(torch.randn(24, 8, generator=g), [i % 4 for i in range(24)], 4)
    net = NWNet(nn.Linear(8, 32), 4, support_dataset=ds, n_shot=2, n_way=4, n_shot_full=6, device="cpu")
    assert net.support_values is None
    net.set_support_values(None)                             # None always clears
    with pytest.raises(NWHipError, match="precompute"):
        net.set_support_values(torch.zeros(24, 3))
    with pytest.raises(NWHipError, match="precompute"):
        net.predict_values(torch.zeros(2, 8))
    with pytest.raises(NWHipError, match="precompute"):
        net.predict_loo_values()
    for name in ("set_support_values", "predict_values", "predict_loo_values"):
        assert "Not in the reference" in getattr(NWNet, name).__doc__


def test_nwnet_refuses_a_sharded_bank():
    from test_sharded_knn_host import _net
    from nwhead_amd.ops import NWHipError
    net = _net()
    hook = lambda *a: None  # noqa: E731  (the compute hooks of the CPU tests: nothing is computed here)
    with torch.no_grad():
        net.precompute_sharded(partial_fn=hook, merge_fn=hook, search_fn=hook, knn_merge_fn=hook)
    with pytest.raises(NWHipError, match="sharded"):
        net.set_support_values(torch.zeros(4, 2))
    with pytest.raises(NWHipError, match="sharded"):
        net.predict_values(torch.zeros(2, 8))
    with pytest.raises(NWHipError, match="sharded"):
        net.predict_loo_values()


def test_nw_head_values_refuses_on_the_host():
    from nwhead_amd import ops
    q, s = torch.zeros(4, 64), torch.zeros(100, 64)
    with pytest.raises(ops.NWHipError, match="MI355X"):
        ops.nw_head_values(q, s, None, torch.zeros(100, 3))          # no CPU path
    with pytest.raises(TypeError, match="SplitBank"):
        ops.BankValues(torch.zeros(100, 3), object())
