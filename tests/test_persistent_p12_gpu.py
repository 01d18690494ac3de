"""The 256-query persistent tile kernel (fused_f16p12.h: eight multiplying waves + four loader waves, pvar 3) against
the 128-query one it is derived from (fused_f16p.h, pvar 2): the same arithmetic element for element, so the outputs
must be bit-equal; and against the fp64 oracle with the bound of test_hip_parity.py::test_persistent_many_tiles.

Both variants are forced through the library's diagnostic knob (nw_debug_set("pvar", ...)).  Shapes too small for the
persistent kernel (fewer than four 64-query tiles per CU) take the one-workgroup-per-tile kernel under either setting.
The oracle is evaluated on the device, in row chunks: its direct-difference form builds a (rows, N, d) fp64 tensor.
"""
import os

import numpy as np
import pytest
import torch

import ws_poison

pytestmark = pytest.mark.gpu

KINDS = ("euclidean", "hypersphere_euclidean", "cosine", "dotproduct", "clip")
RTOL = 1e-5
C = 200


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "run with -m gpu on the MI355X box"
    from nwhead_amd import _lib
    _lib.check(_lib.load().nw_device_check(), "nw_device_check")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from nwhead_amd import ops as o
    return o


@pytest.fixture(scope="module")
def O():
    from oracle import nw_oracle
    return nw_oracle


@pytest.fixture
def pvar():
    """set(v) forces the persistent kernel's tile variant; the knob is unset again after the test."""
    from nwhead_amd import _lib
    _lib.load()
    before = os.environ.get("NW_PVAR")

    def set_(v):
        os.environ["NW_PVAR"] = str(v)
        _lib.sync_knobs()

    yield set_
    if before is None:
        os.environ.pop("NW_PVAR", None)
    else:
        os.environ["NW_PVAR"] = before
    _lib.sync_knobs()


def _oracle_rows(O, q, s, sy, kind, rows):
    """O.nw_head_f64 on the device, `rows` queries at a time."""
    return torch.cat([O.nw_head_f64(q[a:a + rows], s, sy, C, kind) for a in range(0, len(q), rows)])


@pytest.mark.parametrize("d", [96, 512])
@pytest.mark.parametrize("N", [4 * 128 * 8 + 80, 50000])
@pytest.mark.parametrize("B", [256, 300, 1000, 6656])
@pytest.mark.parametrize("sorted_labels", [True, False])
@pytest.mark.parametrize("kind", KINDS)
def test_p12_equals_p2_and_oracle(dev, ops, O, pvar, kind, sorted_labels, B, N, d):
    g = torch.Generator().manual_seed(1000 * B + N + d)
    q = (torch.randn(B, d, generator=g) * 0.7).to(dev)
    s = torch.randn(N, d, generator=g).to(dev)
    sy = torch.arange(N) % C
    sy = (sy.sort().values if sorted_labels else sy[torch.randperm(N, generator=g)]).to(dev)
    cache = ops.SplitBank(s)
    assert cache.split is not None
    ls = torch.tensor(float(np.log(1 / 0.07)), dtype=torch.float32, device=dev) if kind == "clip" else None
    # both variants lay the scratch buffer out alike: without the poison a store that one forgets is filled in by the other
    need = ws_poison.fwd_workspace_bytes(B, N, d, C)
    pvar(2)
    assert ws_poison.poison_cached_workspaces(need, dev) >= need
    out2 = ops.nw_head(q, s, sy, C, kind, ls, support_cache=cache).clone()
    pvar(3)
    assert ws_poison.poison_cached_workspaces(need, dev) >= need
    out3 = ops.nw_head(q, s, sy, C, kind, ls, support_cache=cache).clone()
    torch.cuda.synchronize()
    assert torch.isfinite(out2).all() and torch.isfinite(out3).all()
    assert torch.equal(out3, out2), f"max |diff| {(out3 - out2).abs().max().item():.3e}"
    ref = _oracle_rows(O, q, s, sy, kind, 16 if N * d > 4_000_000 else 256)
    smax = O.scores_f64(q[:64], s, kind, O.CLIP_LOGIT_SCALE_INIT).abs().max().item()
    atol = max(3e-5, 3e-6 * smax)
    np.testing.assert_allclose(out3.cpu().numpy(), ref.cpu().numpy(), rtol=RTOL, atol=atol)
