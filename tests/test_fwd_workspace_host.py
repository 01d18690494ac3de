"""The map of the forward workspace (nw::FwdLayout, nwhead_amd/csrc/fused.hip) through nw_debug_fwd_layout, on the host: no
GPU.  Six areas in a fixed order, each on a multiple of 256 bytes, each starting where the one before ends and the last
ending at nw_fwd_workspace_bytes -- hence pairwise disjoint -- and each at least as large as what its user stores there.
The totals on the golden grid are those of the library before the record existed (tests/golden/h1_workspace_bytes.npz)."""
import ctypes
import itertools
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NW_OK, NW_ERR_INVALID_ARG = 0, -1
MAIN, Q_ROWS, Q_SCALE, Q_NORM2, LSE, SLICES = range(6)


@pytest.fixture(scope="module")
def L():
    from nwhead_amd import _lib
    _lib.load()
    return _lib


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(ROOT, "tests", "golden", "h1_workspace_bytes.npz"))
    ds, Bs, Ns = (z[k].tolist() for k in ("ds", "Bs", "Ns"))
    return {(B, N, d, int(z["C"])): int(z["fwd"][di, bi, ni])
            for di, d in enumerate(ds) for bi, B in enumerate(Bs) for ni, N in enumerate(Ns)}


# few queries over long rows: the shapes at which the sliced aggregation, the query split and the lse slot meet
SLICED = [(B, N, d, C) for B, N, C, d in itertools.product((1, 4, 64), (4096, 50000), (1, 3, 200), (32, 64, 512))]


def check_map(L, B, N, d, C):
    m = L.fwd_layout(B, N, d, C)
    off, size = list(m.off), list(m.bytes)
    assert L.FWD_AREAS == ("main", "q_rows", "q_scale", "q_norm2", "lse", "slices")
    assert all(o % 256 == 0 for o in off), (B, N, d, C, off)
    assert off[MAIN] == 0
    for i in range(1, 6):                                     # the stated order, no gap, no overlap
        assert off[i] == off[i - 1] + size[i - 1], (B, N, d, C, i)
    assert off[SLICES] + size[SLICES] == m.total
    assert m.total == L.load().nw_fwd_workspace_bytes(B, N, d, C)
    assert size[MAIN] >= 4 * B * N
    assert size[Q_ROWS] >= 4 * B * d
    assert size[Q_SCALE] >= 4 * B and size[Q_NORM2] >= 4 * B
    assert size[LSE] >= 4 * B
    assert m.n_slices >= 1
    if m.n_slices == 1:
        assert size[SLICES] == 0
    else:
        assert size[SLICES] >= 4 * m.n_slices * B * (2 + C)
    return m


def test_areas_tile_the_workspace_on_the_golden_grid(L, golden):
    assert len(golden) == 2 * 11 * 20
    for (B, N, d, C), total in golden.items():
        assert check_map(L, B, N, d, C).total == total, (B, N, d, C)


@pytest.mark.parametrize("B,N,d,C", SLICED)
def test_areas_tile_the_workspace_where_the_aggregation_is_sliced(L, B, N, d, C):
    m = check_map(L, B, N, d, C)
    assert m.n_slices > 1 and m.bytes[SLICES] > 0             # B <= 64 and N >= 4096: every shape of this grid is sliced


def test_lse_slot_and_query_norms_do_not_intersect(L):
    """(4, 4096, 64, 3): a = 1024, b = 256, slice = 256.  Subtracting from the total without the slice area put the split
    queries' norm2 array on the very 256 bytes of the log-sum-exp slot."""
    m = L.fwd_layout(4, 4096, 64, 3)
    assert m.n_slices > 1
    norms = range(m.off[Q_NORM2], m.off[Q_NORM2] + m.bytes[Q_NORM2])
    lse = range(m.off[LSE], m.off[LSE] + m.bytes[LSE])
    assert len(norms) and len(lse)
    assert norms.stop <= lse.start or lse.stop <= norms.start


def test_refused_arguments_and_empty_shapes(L):
    lib = L.load()
    m = L.FwdLayout()
    assert lib.nw_debug_fwd_layout(4, 4096, 64, 3, None) == NW_ERR_INVALID_ARG
    for bad in ((-1, 4096, 64, 3), (4, -1, 64, 3), (4, 4096, -64, 3), (4, 4096, 64, -3)):
        assert lib.nw_debug_fwd_layout(*bad, ctypes.byref(m)) == NW_ERR_INVALID_ARG
    for empty in ((0, 4096, 64, 3), (4, 0, 64, 3), (0, 0, 0, 0)):
        ctypes.memset(ctypes.byref(m), 0xFF, ctypes.sizeof(m))
        assert lib.nw_debug_fwd_layout(*empty, ctypes.byref(m)) == NW_OK
        assert bytes(m) == bytes(ctypes.sizeof(m)), empty
