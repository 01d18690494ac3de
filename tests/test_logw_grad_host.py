"""The host-side surface of the learnable support weights (no GPU): the declarations and refusals of nw_bwd_query_logw_f32 /
nw_bwd_logw_workspace_bytes through ctypes, the workspace sizes against the layout worked out by hand, their stand-alone
sanitizer program (tests/sanitize/abi_args_bwd_logw.cpp: a host-only AddressSanitizer + UndefinedBehaviorSanitizer build of
the library's own sources against a HIP runtime stand-in; nothing is loaded into python), the route rule's new fact as a pure
function, and NWNet.set_support_weights(learnable=True) as far as it goes without a bank."""
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
    assert "int nw_bwd_query_logw_f32(" in text and "size_t nw_bwd_logw_workspace_bytes(" in text
    assert "#define NW_ABI_VERSION 2" in text.replace("  ", " ")                 # additions only
    assert "no gradient with respect to row_logw" in text                        # still true of nw_bwd_query_weighted_f32
    sig = _lib().SIGNATURES
    # the weighted backward's arguments with glogw behind gq; the workspace size with want_gq behind row_chunks
    assert len(sig["nw_bwd_query_logw_f32"][1]) == len(sig["nw_bwd_query_weighted_f32"][1]) + 1 == 25
    assert len(sig["nw_bwd_logw_workspace_bytes"][1]) == len(sig["nw_bwd_query_workspace_bytes"][1]) + 1 == 6
    lib = _lib().load()
    assert hasattr(lib, "nw_bwd_query_logw_f32") and hasattr(lib, "nw_bwd_logw_workspace_bytes")
    assert "nw_bwd_query_logw_f32" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_sanitizer_program_builds_and_exits_0():
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "nwhead_amd", "csrc"), "sanitize_bwd_logw", "-j4"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    assert "abi_args_bwd_logw: all argument checks refused as documented" in r.stdout
    assert "runtime error" not in r.stdout + r.stderr and "AddressSanitizer" not in r.stdout + r.stderr


def _aligned(nbytes):
    raw = ctypes.create_string_buffer(nbytes + 16)
    return raw, (ctypes.addressof(raw) + 15) & ~15


@pytest.mark.parametrize("want_gq", [0, 1])
def test_refusals_before_any_launch(want_gq):
    lib = _lib().load()
    B, N, d, C = 8, 1000, 64, 5
    need = lib.nw_bwd_logw_workspace_bytes(B, N, d, C, 0, want_gq)
    assert need > 0
    keep, buf = _aligned(256)           # stands for every device pointer: a refused call reads none of them
    GQ = buf if want_gq else None

    def call(a=buf, lo=buf, hi=buf, sy=buf, lse=buf, out=buf, gout=buf, gq=GQ, ga=buf, ws=buf, ws_bytes=need - 1, B=B, N=N, d=d,
             C=C, exclude=0, q=buf, kind=0, chunks=0):
        return lib.nw_bwd_query_logw_f32(q, buf, buf, buf, sy, a, lo, hi, exclude, lse, out, gout, gq, ga, None, ws, ws_bytes, B, N,
                                         d, C, kind, None, chunks, None)

    assert call(ga=None) == NW_ERR_INVALID_ARG and call(a=None) == NW_ERR_INVALID_ARG      # glogw and row_logw are required
    assert call(ga=None, lo=None, hi=None) == NW_ERR_INVALID_ARG
    assert call(lo=None) == NW_ERR_INVALID_ARG and call(hi=None, exclude=1) == NW_ERR_INVALID_ARG     # half a window
    for win in (dict(), dict(lo=None, hi=None)):
        for exclude in (0, 1):
            kw = dict(exclude=exclude, **win)
            assert call(d=100, **kw) == NW_ERR_UNSUPPORTED
            assert call(N=25, **kw) == NW_ERR_UNSUPPORTED
            assert call(C=0, **kw) == NW_ERR_UNSUPPORTED
            assert call(q=buf + 4, ws_bytes=need, **kw) == NW_ERR_UNSUPPORTED
            assert call(ga=buf + 4, ws_bytes=need, **kw) == NW_ERR_UNSUPPORTED           # a misaligned glogw
            assert call(a=buf + 4, ws_bytes=need, **kw) == NW_ERR_UNSUPPORTED
            if want_gq:
                assert call(gq=buf + 4, ws_bytes=need, **kw) == NW_ERR_UNSUPPORTED
            assert call(**kw) == NW_ERR_WORKSPACE                                        # one byte short
            assert call(ws=None, ws_bytes=need, **kw) == NW_ERR_WORKSPACE
            assert call(ws=buf + 4, ws_bytes=need, **kw) == NW_ERR_UNSUPPORTED
            # B == 0: NW_OK and nothing is touched, glogw included -- the documented choice
            assert call(B=0, **kw) == NW_OK
            assert call(B=0, q=None, sy=None, lse=None, out=None, gout=None, gq=None, ga=None, ws=None, ws_bytes=0,
                        **{**kw, "a": None}) == NW_OK
            for name in ("q", "sy", "lse", "out", "gout"):
                assert call(**{name: None}, **kw) == NW_ERR_INVALID_ARG, name
            assert call(chunks=-1, **kw) == NW_ERR_INVALID_ARG
            assert call(B=-1, **kw) == NW_ERR_INVALID_ARG
            assert call(kind=4, **kw) == NW_ERR_INVALID_ARG                              # clip without its logit scale
            assert call(kind=7, **kw) == NW_ERR_UNSUPPORTED
    # the weights-only size does not serve the call with gq
    if want_gq:
        assert call(ws_bytes=lib.nw_bwd_logw_workspace_bytes(B, N, d, C, 0, 0)) == NW_ERR_WORKSPACE
    header = open(os.path.join(ROOT, "include", "nwhead_hip.h")).read()
    assert "B == 0: NW_OK and NOTHING is" in header
    del keep


def _a256(nfloat):
    return (4 * nfloat + 255) & ~255


def test_workspace_bytes_by_hand():
    """dptab (B,C) | tb (B) | ascale, rqp (chunks,B; with gq) | glsp (chunks,B) | part (chunks,B,d; with gq) | gap
    (query tiles, 64 x row tiles), every area rounded up to 256 bytes."""
    lib = _lib().load()
    # weights only at 256 x 50000 x 512: 4 query tiles, 782 row tiles; chunks fill the chip: ceil(256 / 4) = 64 -> 13 tiles per
    # chunk -> 61 chunks
    B, N, d, C = 256, 50000, 512, 200
    n_q, n_s = 4, 782
    tpc = -(-n_s // 64)
    chunks = -(-n_s // tpc)
    assert (tpc, chunks) == (13, 61)
    want = _a256(B * C) + _a256(B) + _a256(chunks * B) + _a256(n_q * 64 * n_s)
    assert lib.nw_bwd_logw_workspace_bytes(B, N, d, C, 0, 0) == want
    both = lib.nw_bwd_logw_workspace_bytes(B, N, d, C, 0, 1)
    query = lib.nw_bwd_query_workspace_bytes(B, N, d, C, 0)
    assert both == query + _a256(n_q * 64 * n_s)            # the query gradient's areas and the column sums behind them
    assert want < query                                      # no partial gq tiles: several chunks of (B, d) floats less
    assert n_q * 64 * n_s * 4 <= (B * N) // 16 + 64 * 64 * 4 * (n_q + n_s)   # B N / 16 bytes, up to the tile padding
    # with gq and a given chunk count, one slab: 130 x 1000 x 64 in 3 chunks -> 3 query tiles, 16 row tiles, 6 tiles per chunk
    B, N, d, C = 130, 1000, 64, 16
    want = (_a256(B * C) + _a256(B) + 2 * _a256(3 * B) + _a256(3 * B) + _a256(3 * B * d) + _a256(3 * 64 * 16))
    assert lib.nw_bwd_logw_workspace_bytes(B, N, d, C, 3, 1) == want
    assert lib.nw_bwd_logw_workspace_bytes(B, N, d, C, 3, 1) == lib.nw_bwd_query_workspace_bytes(B, N, d, C, 3) + _a256(3 * 64 * 16)
    assert lib.nw_bwd_logw_workspace_bytes(B, N, d, C, 3, 0) == _a256(B * C) + _a256(B) + _a256(3 * B) + _a256(3 * 64 * 16)
    # the chunk count is clamped to the row tiles; outside the regime the size is 0
    assert lib.nw_bwd_logw_workspace_bytes(B, N, d, C, 1000, 0) == lib.nw_bwd_logw_workspace_bytes(B, N, d, C, 16, 0)
    for gq in (0, 1):
        assert lib.nw_bwd_logw_workspace_bytes(0, N, d, C, 0, gq) == 0
        assert lib.nw_bwd_logw_workspace_bytes(B, 25, d, C, 0, gq) == 0
        assert lib.nw_bwd_logw_workspace_bytes(B, N, 100, C, 0, gq) == 0


def test_route_rule_gradient_to_the_weights():
    from nwhead_amd.ops import HEAD_WINDOW_MAX_CLASSES, head_bank_route, head_weighted_route
    base = dict(split=True, sorted_copy=False, shape=(50000, 512), pad=0, width=512, B=256, n_classes=200)
    table = [(base, "fused"),
             ({**base, "shape": (26, 32), "width": 32, "B": 1, "n_classes": 1}, "fused"),
             ({**base, "pad": 12, "width": 500}, "fused"),
             ({**base, "shape": (400000, 256), "width": 256}, "fused"),                 # no size gate
             ({**base, "n_classes": HEAD_WINDOW_MAX_CLASSES}, "fused"),
             ({**base, "split": False}, None),                                           # an fp16 or norms-only bank
             ({**base, "sorted_copy": True}, None),                                      # a class-sorted copy
             ({**base, "shape": (25, 512)}, None),                                       # N <= 25
             ({**base, "shape": (50000, 500), "width": 500}, None),                      # a width that is no multiple of 32
             ({**base, "width": 500}, None),
             ({**base, "B": 0}, None),
             ({**base, "n_classes": HEAD_WINDOW_MAX_CLASSES + 1}, None)]
    for facts, want in table:
        assert head_weighted_route(**facts, grad_logw=True) == want, facts
        assert head_weighted_route(**facts, grad=True, grad_logw=True) == want, facts
        # served exactly where the query gradient is served today
        assert head_weighted_route(**facts, grad_logw=True) == head_weighted_route(**facts, grad=True)
        assert (want == "fused") == (head_bank_route(**facts) == "fused")
        # the forward's rule is what it was
        assert head_weighted_route(**facts) == ("fused" if want == "fused" else "matrix")


class _AnyBank:
    label_max = None
    split, sorted_rows, pad, shape = None, None, 0, (100, 64)

    def matches(self, s):
        return True


def test_refusal_names_the_way_out(monkeypatch):
    """Where the kernel does not serve, the gradient to the weights is refused with the composition through the score matrix
    in the text (a bank without split rows, on the CPU: the refusal comes before anything is launched)."""
    from nwhead_amd import ops
    monkeypatch.setattr(ops, "SplitBank", _AnyBank)
    monkeypatch.setattr(ops, "_need_hip", lambda *a: None)
    q, s, sy = torch.zeros(4, 64), torch.zeros(100, 64), torch.zeros(100, dtype=torch.int64)
    a = torch.zeros(100, requires_grad=True)
    with pytest.raises(ops.NWHipError, match=r"nw_scores \+ a \+ nw_aggregate"):
        ops.nw_head_bank(q, s, sy, 5, _AnyBank(), row_logw=a)
    with pytest.raises(ops.NWHipError, match="no split rows"):
        ops.nw_head_bank(q, s, sy, 5, _AnyBank(), row_logw=a * 2.0)              # a graph tensor asks for it as well


class _DS(torch.utils.data.Dataset):
    def __init__(self, data, targets, C):
        self.data, self.targets, self.num_classes = data, list(targets), C

    def __len__(self):
        return len(self.targets)

    def __getitem__(self, i):
        return self.data[i], self.targets[i]


def test_nwnet_learnable_surface_without_a_bank():
    import inspect
    from nwhead_amd.nwhead.nw import NWNet
    from nwhead_amd.ops import NWHipError
    g = torch.Generator().manual_seed(5)
    targets = [c for c in range(4) for _ in range(6)]
    net = NWNet(nn.Linear(8, 32), 4, support_dataset=_DS(torch.randn(24, 8, generator=g), targets, 4), n_shot=2, n_way=4,
                n_shot_full=6, device="cpu")
    assert inspect.signature(NWNet.set_support_weights).parameters["learnable"].default is False
    assert "support_logw" not in net.state_dict() and "support_logw" not in dict(net.named_parameters())
    assert net.support_weights is None
    with pytest.raises(NWHipError, match="precompute"):
        net.set_support_weights(torch.zeros(24), learnable=True)
    # a bank's features put in place by hand (no kernel runs): what set_support_weights looks at
    net.full_feat, net.full_y = torch.randn(24, 32, generator=g), torch.tensor(targets)
    w = torch.linspace(-1, 1, 24)
    with pytest.raises(ValueError, match="-inf mask outside the parameter"):
        net.set_support_weights(torch.where(torch.arange(24) == 3, torch.tensor(float("-inf")), w), learnable=True)
    assert "support_logw" not in net.state_dict()
    net.set_support_weights(w, learnable=True)
    assert isinstance(net.support_logw, nn.Parameter) and net.support_logw.requires_grad
    assert "support_logw" in net.state_dict() and "support_logw" in dict(net.named_parameters())
    assert torch.equal(net.support_weights, w) and not net.support_weights.requires_grad     # read detached
    assert net._weights_for("forward_bank", graph=True) is net.support_logw
    assert not net._weights_for("predict_loo").requires_grad
    with torch.no_grad():
        net.support_logw.add_(1.0)                                                          # an optimizer step
    assert torch.equal(net.support_weights, w + 1.0)
    # learnable=False is the plain attribute it was; None clears either kind
    net.set_support_weights(w)
    assert "support_logw" not in net.state_dict() and torch.equal(net.support_weights, w)
    assert net._weights_for("forward_bank", graph=True) is net.support_weights
    net.set_support_weights(w, learnable=True)
    net.set_support_weights(None)
    assert net.support_weights is None and "support_logw" not in net.state_dict()
    assert "weight decay" in NWNet.set_support_weights.__doc__ and "precompute()" in NWNet.set_support_weights.__doc__
