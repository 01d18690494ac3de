"""The tile epilogue of the 256-query persistent kernel (fused_f16p12.h, pvar 3) against the 128-query kernel it is
derived from (fused_f16p.h, pvar 2), bit for bit, on the cases its partial stores and lane-group reductions depend on:

  * support tiles with exactly 1, 2, 3 and more than 3 (also more than 16) runs of equal labels, a run boundary inside a
    16-row block and one on a block edge, runs that continue across a tile edge and runs that start on it;
  * a ragged last support tile (N not a multiple of 128) and a whole one;
  * B not a multiple of 256 and not a multiple of 16, so that `b < B` cuts inside a lane group's 16 rows;
  * all five score kinds;
  * the partial-output entry point (nw_fwd_partial_f32 through ShardedBank._partial): the packed row [m | den | num]
    itself is compared, so a value stored into another array's slot cannot hide behind the merge to log-probabilities.

Both variants are forced through NW_PVAR, as in test_persistent_p12_gpu.py.  The shapes are the smallest that take the
persistent kernel (four 64-query tiles per CU); each test asserts that its shape does, and that the forced variant is the one
the library plans (persistent_schedule.assert_persistent: nw_debug_fwd_plan with the device's CU count).
"""
import os

import numpy as np
import pytest
import torch

import ws_poison
from persistent_schedule import assert_persistent

pytestmark = pytest.mark.gpu

KINDS = ("euclidean", "hypersphere_euclidean", "cosine", "dotproduct", "clip")
C = 200
D = 96
BS = 128   # support rows per tile of both kernels
# (B, N): B % 256, B % 16 and N % 128 are zero only where that is the case under test
SHAPES = [(520, 16500),    # B = 2 * 256 + 8: the last lane group's segment is cut after 8 rows; last tile 116 rows
          (300, 26300),    # B = 256 + 44: one whole wave, one cut inside its second query block; last tile 60 rows
          (512, 16384)]    # whole tiles on both sides
# run boundaries (rows of the tile) per tile type, cycled over the support tiles
TILE_CUTS = [[], [37], [48], [16, 100], [5, 6], [], [10, 37, 64, 90], list(range(3, 128, 6)), [127]]


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


def crafted_labels(N):
    """Labels whose runs are cut per support tile as TILE_CUTS says; every third tile also starts a new run on its edge."""
    y = np.empty(N, dtype=np.int64)
    lab = 0
    for t in range((N + BS - 1) // BS):
        if t % 3 == 0:
            lab += 1
        cuts = set(TILE_CUTS[t % len(TILE_CUTS)])
        for r in range(min(BS, N - t * BS)):
            if r in cuts:
                lab += 1
            y[t * BS + r] = (7 * lab) % C   # consecutive runs differ: 7 and C are coprime
    return torch.from_numpy(y)


def runs_per_tile(y):
    y = y.numpy()
    return [1 + int(np.count_nonzero(np.diff(y[a:a + BS]))) for a in range(0, len(y), BS)]


def test_crafted_labels_cover_every_run_path():
    for _, N in SHAPES:
        y = crafted_labels(N)
        n = set(runs_per_tile(y))
        assert {1, 2, 3} <= n and any(3 < k <= 16 for k in n) and any(k > 16 for k in n), sorted(n)
        # a run that crosses a tile edge, and one that starts on it
        yn = y.numpy()
        first = yn[BS::BS]                       # first rows of tiles 1, 2, ...
        edges = first != yn[BS - 1::BS][:len(first)]
        assert edges.any() and not edges.all()


def _inputs(dev, B, N, labels):
    g = torch.Generator().manual_seed(7 * B + N)
    q = (torch.randn(B, D, generator=g) * 0.7).to(dev)
    s = torch.randn(N, D, generator=g).to(dev)
    sy = crafted_labels(N) if labels == "crafted" else (torch.arange(N) % C).sort().values
    return q, s, sy.to(dev)


def _assert_persistent(dev, B, N, variant=None):
    assert_persistent(B, N, D, torch.cuda.get_device_properties(dev).multi_processor_count, variant=variant)


def _logit_scale(kind, dev):
    return torch.tensor(float(np.log(1 / 0.07)), dtype=torch.float32, device=dev) if kind == "clip" else None


@pytest.mark.parametrize("labels", ["crafted", "sorted"])
@pytest.mark.parametrize("B,N", SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_p12_epilogue_log_probs_equal_p2(dev, ops, pvar, kind, B, N, labels):
    _assert_persistent(dev, B, N)
    q, s, sy = _inputs(dev, B, N, labels)
    cache = ops.SplitBank(s)
    assert cache.split is not None
    ls = _logit_scale(kind, dev)
    # both variants lay the scratch buffer out alike: without the poison a store that one forgets is filled in by the other
    need = ws_poison.fwd_workspace_bytes(B, N, D, C)
    pvar(2)
    _assert_persistent(dev, B, N, variant=2)
    assert ws_poison.poison_cached_workspaces(need, dev) >= need
    out2 = ops.nw_head(q, s, sy, C, kind, ls, support_cache=cache).clone()
    pvar(3)
    _assert_persistent(dev, B, N, variant=3)
    assert ws_poison.poison_cached_workspaces(need, dev) >= need
    out3 = ops.nw_head(q, s, sy, C, kind, ls, support_cache=cache).clone()
    torch.cuda.synchronize()
    assert out2.shape == (B, C) and not torch.isnan(out2).any()
    assert torch.isfinite(out2).all() and torch.isfinite(out3).all()
    assert torch.equal(out3, out2), f"max |diff| {(out3 - out2).abs().max().item():.3e}"


@pytest.mark.parametrize("B,N", SHAPES[:2])
@pytest.mark.parametrize("kind", KINDS)
def test_p12_epilogue_packed_partials_equal_p2(dev, pvar, kind, B, N):
    from nwhead_amd.sharded import ShardedBank
    _assert_persistent(dev, B, N)
    q, s, sy = _inputs(dev, B, N, "crafted")
    bank = ShardedBank(s, sy, C, kind, _logit_scale(kind, dev))
    assert bank.cache is not None and bank.cache.split is not None
    rows = {}
    need = ws_poison.fwd_workspace_bytes(B, N, D, bank.CL)
    for v in (2, 3):
        pvar(v)
        _assert_persistent(dev, B, N, variant=v)
        # the bank's own scratch buffer (kept from call to call, never cleared) is the one in use; the shared one is poisoned
        # too so that nothing can come from it, and may rightly be empty here: its byte count is not asserted
        bank._ws = ws_poison.poisoned_workspace(need, dev)
        ws_poison.poison_cached_workspaces()
        packed = torch.full((bank.row_len(B),), -7.0, dtype=torch.float32, device=dev)
        bank._partial(packed, q)
        torch.cuda.synchronize()
        rows[v] = packed.clone()
    m2, den2, num2 = rows[2][:B], rows[2][B:2 * B], rows[2][2 * B:]
    m3, den3, num3 = rows[3][:B], rows[3][B:2 * B], rows[3][2 * B:]
    assert not torch.isnan(rows[2]).any() and (den2 > 0).all() and (num2 >= 0).all()
    assert torch.isfinite(rows[2]).all() and torch.isfinite(rows[3]).all()
    assert torch.equal(m3, m2), f"m: {(m3 != m2).sum().item()} of {B} differ"
    assert torch.equal(den3, den2), f"den: {(den3 != den2).sum().item()} of {B} differ"
    assert torch.equal(num3, num2), f"num: {(num3 != num2).sum().item()} of {B * C} differ"
    assert torch.equal(rows[3], rows[2])
