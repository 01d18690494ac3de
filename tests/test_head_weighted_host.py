"""The host-side surface of the support weights (no GPU): the declarations and refusals of nw_fwd_weighted_f32 /
nw_bwd_query_weighted_f32 through ctypes, their stand-alone sanitizer program (tests/sanitize/abi_args_fwd_weighted.cpp: a
host-only AddressSanitizer + UndefinedBehaviorSanitizer build of the library's own sources against a HIP runtime stand-in;
nothing is loaded into python), the route rule as a pure function, ops.class_balance_logw against a numpy restatement, and
FullDataset / NWNet(balance_full="weights") on a toy imbalanced dataset."""
import ctypes
import os
import subprocess

import numpy as np
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
    assert "int nw_fwd_weighted_f32(" in text and "int nw_bwd_query_weighted_f32(" in text
    assert "#define NW_ABI_VERSION 2" in text.replace("  ", " ")
    assert "no gradient with respect to row_logw" in text
    # the window entries' arguments with the weights in front of the window
    assert len(_lib().SIGNATURES["nw_fwd_weighted_f32"][1]) == len(_lib().SIGNATURES["nw_fwd_window_f32"][1]) + 1 == 20
    assert len(_lib().SIGNATURES["nw_bwd_query_weighted_f32"][1]) == len(_lib().SIGNATURES["nw_bwd_query_f32"][1]) + 1 == 24


def test_sanitizer_program_builds_and_exits_0():
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "nwhead_amd", "csrc"), "sanitize_fwd_weighted", "-j4"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    assert "abi_args_fwd_weighted: all argument checks refused as documented" in r.stdout
    assert "runtime error" not in r.stdout + r.stderr and "AddressSanitizer" not in r.stdout + r.stderr


def _aligned(nbytes):
    raw = ctypes.create_string_buffer(nbytes + 16)
    return raw, (ctypes.addressof(raw) + 15) & ~15


def test_forward_refusals_before_any_launch():
    lib = _lib().load()
    B, N, d, C = 8, 1000, 64, 5
    need = lib.nw_fwd_workspace_bytes(B, N, d, C)
    assert need > 0
    keep, buf = _aligned(256)           # stands for every device pointer: a refused call reads none of them

    def call(a=buf, lo=buf, hi=buf, sy=buf, out=buf, ws=buf, ws_bytes=need - 1, B=B, N=N, d=d, C=C, exclude=0, q=buf, kind=0):
        return lib.nw_fwd_weighted_f32(q, buf, buf, buf, sy, a, lo, hi, exclude, out, None, ws, ws_bytes, B, N, d, C, kind, None, None)

    assert call(a=None) == NW_ERR_INVALID_ARG                                    # the weights are required
    assert call(a=None, lo=None, hi=None) == NW_ERR_INVALID_ARG
    assert call(lo=None) == NW_ERR_INVALID_ARG and call(hi=None, exclude=1) == NW_ERR_INVALID_ARG     # half a window
    for win in (dict(), dict(lo=None, hi=None)):                                 # with a window and without
        for exclude in (0, 1):
            kw = dict(exclude=exclude, **win)
            assert call(d=100, **kw) == NW_ERR_UNSUPPORTED                       # nw_fwd_window_f32's regime
            assert call(d=16, **kw) == NW_ERR_UNSUPPORTED
            assert call(N=25, **kw) == NW_ERR_UNSUPPORTED
            assert call(C=0, **kw) == NW_ERR_UNSUPPORTED
            assert call(q=buf + 4, ws_bytes=need, **kw) == NW_ERR_UNSUPPORTED
            assert call(a=buf + 4, ws_bytes=need, **kw) == NW_ERR_UNSUPPORTED    # float4 reads of the weights
            assert call(**kw) == NW_ERR_WORKSPACE                                # nw_fwd_workspace_bytes, one byte short
            assert call(ws=None, ws_bytes=need, **kw) == NW_ERR_WORKSPACE
            assert call(ws=buf + 4, ws_bytes=need, **kw) == NW_ERR_UNSUPPORTED
            assert call(B=0, **kw) == NW_OK
            assert call(B=0, q=None, sy=None, out=None, ws=None, ws_bytes=0, **{**kw, "a": None}) == NW_OK
            assert call(sy=None, **kw) == NW_ERR_INVALID_ARG
            assert call(out=None, **kw) == NW_ERR_INVALID_ARG
            assert call(q=None, **kw) == NW_ERR_INVALID_ARG
            assert call(B=-1, **kw) == NW_ERR_INVALID_ARG
            assert call(kind=4, **kw) == NW_ERR_INVALID_ARG                      # clip without its logit scale
            assert call(kind=7, **kw) == NW_ERR_UNSUPPORTED
    from nwhead_amd.ops import HEAD_WINDOW_MAX_CLASSES
    assert call(C=HEAD_WINDOW_MAX_CLASSES, ws_bytes=0) == NW_ERR_WORKSPACE and call(C=HEAD_WINDOW_MAX_CLASSES + 1, ws_bytes=0) == NW_ERR_UNSUPPORTED
    del keep


def test_backward_refusals_before_any_launch():
    lib = _lib().load()
    B, N, d, C = 8, 1000, 64, 5
    need = lib.nw_bwd_query_workspace_bytes(B, N, d, C, 0)
    assert need > 0
    keep, buf = _aligned(256)

    def call(a=buf, lo=buf, hi=buf, sy=buf, lse=buf, out=buf, gout=buf, gq=buf, ws=buf, ws_bytes=need - 1, B=B, N=N, d=d, C=C,
             exclude=0, q=buf, kind=0, chunks=0):
        return lib.nw_bwd_query_weighted_f32(q, buf, buf, buf, sy, a, lo, hi, exclude, lse, out, gout, gq, None, ws, ws_bytes, B, N, d,
                                             C, kind, None, chunks, None)

    assert call(a=None) == NW_ERR_INVALID_ARG
    assert call(lo=None) == NW_ERR_INVALID_ARG and call(hi=None) == NW_ERR_INVALID_ARG
    for win in (dict(), dict(lo=None, hi=None)):
        for exclude in (0, 1):
            kw = dict(exclude=exclude, **win)
            assert call(d=100, **kw) == NW_ERR_UNSUPPORTED
            assert call(N=25, **kw) == NW_ERR_UNSUPPORTED
            assert call(C=0, **kw) == NW_ERR_UNSUPPORTED
            assert call(q=buf + 4, ws_bytes=need, **kw) == NW_ERR_UNSUPPORTED
            assert call(gq=buf + 4, ws_bytes=need, **kw) == NW_ERR_UNSUPPORTED
            assert call(a=buf + 4, ws_bytes=need, **kw) == NW_ERR_UNSUPPORTED
            assert call(**kw) == NW_ERR_WORKSPACE
            assert call(ws=None, ws_bytes=need, **kw) == NW_ERR_WORKSPACE
            assert call(B=0, **kw) == NW_OK
            for name in ("q", "sy", "lse", "out", "gout", "gq"):
                assert call(**{name: None}, **kw) == NW_ERR_INVALID_ARG, name
            assert call(chunks=-1, **kw) == NW_ERR_INVALID_ARG
            assert call(kind=4, **kw) == NW_ERR_INVALID_ARG
            assert call(kind=7, **kw) == NW_ERR_UNSUPPORTED
    del keep


def test_route_rule():
    from nwhead_amd.ops import HEAD_WINDOW_MAX_CLASSES, head_weighted_route, head_window_route
    base = dict(split=True, sorted_copy=False, shape=(50000, 512), pad=0, width=512, B=256, n_classes=200)
    variants = [base, {**base, "shape": (26, 32), "width": 32, "B": 1, "n_classes": 1}, {**base, "pad": 12, "width": 500},
                {**base, "split": False}, {**base, "sorted_copy": True}, {**base, "shape": (25, 512)}, {**base, "width": 500},
                {**base, "B": 0}, {**base, "n_classes": 0}, {**base, "n_classes": HEAD_WINDOW_MAX_CLASSES},
                {**base, "n_classes": HEAD_WINDOW_MAX_CLASSES + 1}, {**base, "shape": (50000, 500), "width": 500}]
    seen = set()
    for facts in variants:
        window_route = head_window_route(**facts)
        seen.add(window_route)
        # fused exactly when the windowed head is; the forward's other route is the matrix, the gradient has none
        assert head_weighted_route(**facts) == window_route
        assert head_weighted_route(**facts, grad=True) == ("fused" if window_route == "fused" else None)
    assert seen == {"fused", "matrix"}
    assert head_weighted_route(**base) == "fused" and head_weighted_route(**{**base, "split": False}) == "matrix"


def test_class_balance_logw():
    from nwhead_amd.ops import class_balance_logw
    rng = np.random.default_rng(3)
    C = 7
    y = rng.integers(0, C, 500)
    y[y == 4] = 5                                    # a class without rows
    got = class_balance_logw(torch.from_numpy(y), C)
    assert got.dtype == torch.float32 and got.shape == (500,)
    counts = np.bincount(y, minlength=C)
    np.testing.assert_allclose(got.numpy(), np.log(1.0 / C / counts[y]), rtol=1e-6)
    mass = np.bincount(y, weights=np.exp(got.double().numpy()), minlength=C)
    np.testing.assert_allclose(mass[counts > 0], 1.0 / C, rtol=1e-6)      # the weights of a class sum to its prior
    prior = rng.random(C) + 0.1
    prior /= prior.sum()
    got = class_balance_logw(torch.from_numpy(y), C, prior=torch.from_numpy(prior))
    np.testing.assert_allclose(got.numpy(), np.log(prior[y] / counts[y]), rtol=1e-6)
    mass = np.bincount(y, weights=np.exp(got.double().numpy()), minlength=C)
    np.testing.assert_allclose(mass[counts > 0], prior[counts > 0], rtol=1e-6)
    # labels outside [0, C) are rows the kernels skip: -inf
    got = class_balance_logw(torch.tensor([0, 0, 1, -1, 9]), 2)
    assert got[3:].tolist() == [float("-inf")] * 2
    np.testing.assert_allclose(got[:3].numpy(), np.log([0.25, 0.25, 0.5]), rtol=1e-6)
    with pytest.raises(ValueError):
        class_balance_logw(torch.tensor([0, 1]), 2, prior=torch.ones(3))


class _DS(torch.utils.data.Dataset):
    def __init__(self, data, targets, C):
        self.data, self.targets, self.num_classes = data, list(targets), C

    def __len__(self):
        return len(self.targets)

    def __getitem__(self, i):
        return self.data[i], self.targets[i]


def _toy(counts):
    g = torch.Generator().manual_seed(5)
    targets = [c for c, n in enumerate(counts) for _ in range(n)]
    targets = [targets[i] for i in torch.randperm(len(targets), generator=g).tolist()]
    return _DS(torch.randn(len(targets), 8, generator=g), targets, len(counts))


def test_full_dataset_keeps_every_class():
    from nwhead_amd.nwhead.utils import FullDataset
    from nwhead_amd.ops import class_balance_logw
    counts = [40, 7, 25, 3]
    ds = _toy(counts)
    by_class = [[i for i, t in enumerate(ds.targets) if t == c] for c in range(len(counts))]
    # the default is what it was: every class cut to the rarest class's count (and to n_shot_full)
    assert FullDataset(ds, 100).keys == [i for ix in by_class for i in ix[:3]]
    assert FullDataset(ds, 2).keys == [i for ix in by_class for i in ix[:2]]
    assert FullDataset(ds, 100, balance="truncate").keys == FullDataset(ds, 100).keys
    # "weights": the first min(n_shot_full, n_c) rows of every class, classes in ascending order
    full = FullDataset(ds, 100, balance="weights")
    assert full.keys == [i for ix in by_class for i in ix]
    capped = FullDataset(ds, 10, balance="weights")
    assert capped.keys == [i for ix in by_class for i in ix[:10]] and len(capped) == 10 + 7 + 10 + 3
    assert [full[k][1] for k in range(len(full))] == sorted(ds.targets)
    with pytest.raises(ValueError):
        FullDataset(ds, 10, balance="other")
    # the weights NWNet sets over such a bank: every class sums to the flat prior
    y = torch.tensor([capped[k][1] for k in range(len(capped))])
    w = class_balance_logw(y, len(counts)).double().exp()
    np.testing.assert_allclose(torch.zeros(4, dtype=torch.float64).index_add_(0, y, w).numpy(), 0.25, rtol=1e-6)


def test_nwnet_balance_full():
    from nwhead_amd.nwhead.nw import NWNet
    from nwhead_amd.ops import NWHipError
    counts = [40, 7, 25, 3]
    ds = _toy(counts)
    mk = lambda **kw: NWNet(nn.Linear(8, 32), len(counts), support_dataset=ds, n_shot=2, n_way=len(counts), n_shot_full=30,  # noqa: E731
                            device="cpu", **kw)
    default = mk()
    assert default.balance_full == "truncate" and default.support_weights is None
    assert [len(d) for d in default.support_eval.full_datasets] == [3 * len(counts)]
    weights = mk(balance_full="weights")
    assert [len(d) for d in weights.support_eval.full_datasets] == [30 + 7 + 25 + 3]
    assert weights.support_weights is None                   # set by precompute(), over the bank it builds
    with pytest.raises(ValueError, match="balance_full"):
        mk(balance_full="both")
    # no bank yet: nothing to weight; None always clears
    with pytest.raises(NWHipError, match="precompute"):
        weights.set_support_weights(torch.zeros(65))
    weights.set_support_weights(None)
    assert "get_neighbors" in NWNet.set_support_weights.__doc__ and "explain" in NWNet.set_support_weights.__doc__


def test_set_support_weights_refuses_a_sharded_bank():
    from test_sharded_knn_host import _net
    from nwhead_amd.ops import NWHipError
    net = _net()
    hook = lambda *a: None  # noqa: E731  (the compute hooks of the CPU tests: nothing is computed here)
    with torch.no_grad():
        net.precompute_sharded(partial_fn=hook, merge_fn=hook, search_fn=hook, knn_merge_fn=hook)
    with pytest.raises(NWHipError, match="sharded"):
        net.set_support_weights(torch.zeros(4))


def test_nw_head_refuses_what_the_weights_cannot_serve():
    from nwhead_amd import ops

    class AnyBank:
        label_max = None

        def matches(self, s):
            return True

    q, s, sy = torch.zeros(4, 64), torch.zeros(100, 64), torch.zeros(100, dtype=torch.int64)
    a = torch.zeros(100)
    with pytest.raises(ValueError, match="support_cache"):
        ops.nw_head(q, s, sy, 5, row_logw=a)
    with pytest.raises(ValueError, match="no gradients"):
        ops.nw_head(q.clone().requires_grad_(True), s, sy, 5, support_cache=AnyBank(), row_logw=a)
    with pytest.raises(ValueError, match="return_weights"):
        ops.nw_head(q, s, sy, 5, return_weights=True, support_cache=AnyBank(), row_logw=a)
