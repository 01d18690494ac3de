"""The launch decision of the fused head (plan_fused, nwhead_amd/csrc/fused.hip) through nw_debug_fwd_plan, on the host: no
GPU, CU count given as 256.  The expected values were derived by hand from the rules as they stood inline in the launchers
before plan_fused existed (pick_rs, the persistent predicate, the raw-or-split-queries rule, the MODE / OUT ladder, the tile
variant and workgroup count of the persistent launch); the workspace sizes are those the library of the commit before
returned (tests/golden/h1_workspace_bytes.npz, recorded by tests/golden/record_workspace_bytes.py from THAT build)."""
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODE = {"REG": 0, "DMA": 1, "DMA_SN": 2, "F16": 3, "F16Q": 4}
OUT = {"NONE": 0, "SCORES": 1, "CAND": 2}
NW_OK, NW_ERR_INVALID_ARG, NW_ERR_UNSUPPORTED = 0, -1, -2
D, C, CUS = 512, 200, 256


@pytest.fixture(scope="module")
def L():
    from nwhead_amd import _lib
    _lib.load()
    return _lib


def plan(L, B, N, d=D, **kw):
    kw.setdefault("cus", CUS)
    return L.fwd_plan(B, N, d, C, **kw)


def test_split_small_grid_runs_raw_queries_one_workgroup_per_tile(L):
    p = plan(L, 256, 10000)
    assert (p.status, p.rs, p.bs, p.n_stiles, p.n_qtiles, p.grid) == (NW_OK, 10, 160, 63, 4, 256)
    assert not p.persistent and not p.split_queries and not p.run_tables and p.dma
    assert (p.mode, p.out) == (MODE["F16Q"], OUT["NONE"])


def test_split_large_grid_takes_the_256_query_persistent_kernel(L):
    p = plan(L, 256, 50000)
    assert (p.status, p.rs, p.bs, p.n_stiles, p.grid) == (NW_OK, 8, 128, 391, 1568)
    assert p.persistent and p.run_tables and p.split_queries
    assert (p.variant, p.workgroups, p.qgroup) == (3, 256, 4)
    assert p.lds_bytes == 158208                      # PipeCfg<128, 256, 8, 4, 3>::LDS_BYTES (profiles/r07_persistent_refactor.md)


@pytest.mark.parametrize("outputs,k,out", [("scores", 0, "SCORES"), ("candidates", 10, "CAND")])
def test_scores_and_candidates_stay_off_the_persistent_kernel(L, outputs, k, out):
    p = plan(L, 256, 50000, outputs=outputs, k=k)
    assert (p.status, p.rs, p.n_stiles, p.grid) == (NW_OK, 8, 391, 1568)
    assert not p.persistent and not p.run_tables and p.split_queries
    assert (p.mode, p.out) == (MODE["F16"], OUT[out])
    assert (p.variant, p.workgroups, p.qgroup) == (0, 0, 0)


def test_split_queries_once_the_grid_passes_three_workgroups_per_two_cus(L):
    p = plan(L, 64, 50000)
    assert (p.status, p.rs, p.n_stiles, p.grid) == (NW_OK, 8, 391, 392)
    assert 2 * p.grid > 3 * CUS and p.grid < 4 * CUS
    assert not p.persistent and p.split_queries
    assert (p.mode, p.out) == (MODE["F16"], OUT["NONE"])


@pytest.mark.parametrize("B,grid,variant,wgs,qgroup", [(130, 1176, 1, 512, 8), (384, 2352, 2, 256, 8)])
def test_persistent_variant_follows_the_padding_of_the_query_tiles(L, B, grid, variant, wgs, qgroup):
    p = plan(L, B, 50000)
    assert (p.status, p.rs, p.n_stiles, p.grid) == (NW_OK, 8, 391, grid)
    assert p.persistent and p.split_queries and p.run_tables
    assert (p.variant, p.workgroups, p.qgroup) == (variant, wgs, qgroup)
    assert p.lds_bytes == {1: 79872, 2: 138752}[variant]   # PCfg<8, 1, true> / PCfg<8, 2, false>


@pytest.mark.parametrize("kind,mode", [("euclidean", "DMA_SN"), ("dotproduct", "DMA")])
def test_fp32_large_grid_runs_80_row_tiles_on_the_dma_loaders(L, kind, mode):
    p = plan(L, 2048, 50000, form="fp32", kind=kind)
    assert (p.status, p.rs, p.bs, p.n_stiles) == (NW_OK, 5, 80, 625)
    assert not p.persistent and not p.split_queries and not p.run_tables and p.dma
    assert (p.mode, p.out) == (MODE[mode], OUT["NONE"])
    assert plan(L, 2048, 50000, form="fp32", kind=kind, norms=False).mode == MODE["DMA"]


def test_fp32_unaligned_d_runs_even_tiles_on_the_register_loaders(L):
    p = plan(L, 64, 1000, d=100, form="fp32")
    assert p.status == NW_OK and p.rs % 2 == 0 and not p.dma
    assert not p.persistent and not p.split_queries
    assert (p.mode, p.out) == (MODE["REG"], OUT["NONE"])


@pytest.mark.parametrize("B,N", [(8, 26), (256, 50000), (4096, 400000)])
def test_half_form_is_the_256_query_kernel_at_every_size(L, B, N):
    p = plan(L, B, N, form="half")
    assert (p.status, p.rs, p.bs, p.n_stiles) == (NW_OK, 8, 128, (N + 127) // 128)
    assert p.persistent and p.variant == 3 and p.split_queries and p.run_tables
    assert (p.workgroups, p.qgroup, p.lds_bytes) == (256, 4, 158208)


@pytest.mark.parametrize("wgs,want", [(0, 256), (248, 248), (250, 248), (4, 256), (264, 256)])
def test_persistent_wgs_caps_the_workgroups_in_multiples_of_eight(L, wgs, want):
    assert plan(L, 256, 50000, persistent_wgs=wgs).workgroups == want
    assert plan(L, 256, 50000, form="half", persistent_wgs=wgs).workgroups == want
    assert plan(L, 130, 50000, persistent_wgs=wgs).workgroups == 2 * want       # variant 1: two per CU


def test_statuses_of_the_combinations_the_launchers_refuse(L):
    assert plan(L, 256, 50000, norms=False).status == NW_ERR_INVALID_ARG                         # split operands without norms
    assert plan(L, 256, 50000, form="fp32", outputs="candidates", k=10).status == NW_ERR_INVALID_ARG
    assert plan(L, 256, 50000, form="half", outputs="scores").status == NW_ERR_UNSUPPORTED
    assert plan(L, 256, 50000, d=100, form="half").status == NW_ERR_UNSUPPORTED
    assert plan(L, 1 << 30, 50000).status == NW_ERR_UNSUPPORTED
    lib = L.load()
    import ctypes
    p = ctypes.byref(L.FwdPlan())
    assert lib.nw_debug_fwd_plan(256, 50000, D, C, 1, 0, 0, 1, 0, 0, CUS, None) == NW_ERR_INVALID_ARG
    assert lib.nw_debug_fwd_plan(-1, 50000, D, C, 1, 0, 0, 1, 0, 0, CUS, p) == NW_ERR_INVALID_ARG
    assert lib.nw_debug_fwd_plan(256, 50000, D, C, 3, 0, 0, 1, 0, 0, CUS, p) == NW_ERR_INVALID_ARG     # unknown form
    assert lib.nw_debug_fwd_plan(256, 50000, D, C, 1, 0, 0, 1, 9, 0, CUS, p) == NW_ERR_UNSUPPORTED     # unknown kind


def _restore_tile_rs(L):
    assert L.load().nw_debug_set(b"tile_rs", L._knob_state.get("tile_rs", -2 ** 31)) == NW_OK   # what sync_knobs last set


def test_forced_tile_height_12_has_no_candidate_form(L):
    lib = L.load()
    try:
        assert lib.nw_debug_set(b"tile_rs", 12) == NW_OK
        p = plan(L, 256, 50000, outputs="candidates", k=10)
        assert p.rs == 12 and p.status == NW_ERR_UNSUPPORTED
        assert lib.nw_knn_workspace_bytes(256, 50000, D, 10) == 0
        assert plan(L, 256, 50000, d=100, form="fp32").rs == 12
    finally:
        _restore_tile_rs(L)
    assert plan(L, 256, 50000, outputs="candidates", k=10).status == NW_OK
    assert lib.nw_knn_workspace_bytes(256, 50000, D, 10) > 0


def test_odd_tile_height_needs_the_dma_loaders(L):
    lib = L.load()
    try:
        assert lib.nw_debug_set(b"tile_rs", 5) == NW_OK
        assert plan(L, 64, 1000, d=100, form="fp32").status == NW_ERR_UNSUPPORTED
        assert plan(L, 64, 1000, d=128, form="fp32").status == NW_OK
    finally:
        _restore_tile_rs(L)


def test_workspace_sizes_are_those_of_the_library_before_the_plan(L):
    lib = L.load()
    z = np.load(os.path.join(ROOT, "tests", "golden", "h1_workspace_bytes.npz"))
    Ns, Bs, ks, ds, Cz = (z[k].tolist() for k in ("Ns", "Bs", "ks", "ds", "C"))
    grids = open(os.path.join(ROOT, "tests", "test_knn_fused_host.py")).read()
    assert all(f"= {g}\n" in grids for g in (Ns, Bs, ks)), "the fixture's grid is no longer the grid of test_knn_fused_host.py"
    for di, d in enumerate(ds):
        for bi, B in enumerate(Bs):
            for ni, N in enumerate(Ns):
                assert lib.nw_fwd_workspace_bytes(B, N, d, Cz) == z["fwd"][di, bi, ni], (B, N, d)
                for ki, k in enumerate(ks):
                    assert lib.nw_knn_workspace_bytes(B, N, d, k) == z["knn"][di, bi, ni, ki], (B, N, d, k)
    n0 = int(z["stretch_N0"])
    for i, want in enumerate(z["stretch"].tolist()):
        assert lib.nw_knn_workspace_bytes(256, n0 + i, 512, 10) == want, n0 + i
