"""A Python model of the tile order of the persistent split-fp16 kernels (PersistentTiles::decode() in
nwhead_amd/csrc/persistent_pipe.h, used by fused_f16p.h and fused_f16p12.h) and of the plan's workgroup count
(plan_fused in fused.hip), and the shapes of the order edges that test_persistent_schedule_gpu.py derives from them.  A plain
helper module: test_persistent_schedule_model.py checks the model on the CPU, the GPU tests use it to state what their shapes
mean -- and assert_persistent() asks the library itself which route a shape takes.
"""

BS = 128                                        # support rows per tile, every persistent variant
BQP = {0: 64, 1: 64, 2: 128, 3: 256}            # query rows per tile, by NW_PVAR
QG_DEFAULT = 8                                  # plan_fused (fused.hip) when NW_QG is unset


def n_local(n_stiles, n_qtiles, xcd):
    """Tiles on the list of XCD `xcd`."""
    return (n_stiles >> 3) * n_qtiles + (n_stiles & 7) * ((n_qtiles - xcd + 7) >> 3)


def decode(L, xcd, n_stiles, n_qtiles, qg):
    """PersistentTiles::decode() (persistent_pipe.h, both persistent kernels): entry L of XCD xcd's list -> (qt, st)."""
    ns_x = n_stiles >> 3
    n_full = ns_x * n_qtiles
    nq_x = (n_qtiles - xcd + 7) >> 3
    if L >= n_full:                              # leftover support tiles, dealt by query tile, support-tile major
        r = L - n_full
        j = r // nq_x
        return xcd + 8 * (r - j * nq_x), 8 * ns_x + j
    grp_tiles = qg * ns_x
    gi = L // grp_tiles
    r = L - gi * grp_tiles
    g = min(qg, n_qtiles - gi * qg)
    stl = r // g
    return gi * qg + (r - stl * g), stl * 8 + xcd


def kernel_qg(pvar, qg):
    """The group size the kernel gets: NW_QG in 1..64, else 8; the 256-query kernel takes half, at least 1."""
    v = qg if (qg is not None and 1 <= qg <= 64) else QG_DEFAULT
    return max(1, v // 2) if pvar == 3 else v


def workgroups(pvar, cus, wgs):
    """FusedPlan.workgroups (plan_fused): `wgs` rounded down to a multiple of 8, used when it is in [8, CUs); two per CU for pvar 1."""
    n = cus & ~7
    cap = wgs & ~7
    if 8 <= cap < n:
        n = cap
    return 2 * n if pvar == 1 else n


def assert_persistent(B, N, d, cus, variant=None, wgs=0, C=200):
    """The library's own launch decision (nw_debug_fwd_plan: plan_fused with the knobs as they are set NOW) for a split-operand
    forward of this shape on `cus` CUs takes the persistent kernel -- of tile variant `variant`, where the test forces one.
    Returns the plan."""
    from nwhead_amd import _lib
    p = _lib.fwd_plan(B, N, d, C, form="split", persistent_wgs=wgs, cus=cus)
    assert p.status == 0 and p.persistent, \
        f"B={B} N={N} d={d}: plan_fused does not take the persistent kernel on {cus} CUs (status {p.status}, rs {p.rs}, grid {p.grid})"
    if variant is not None:
        assert p.variant == variant, f"B={B} N={N} d={d}: tile variant {p.variant}, not the forced {variant}"
    return p


EDGES = ("fewer_than_8_stiles", "stiles_0_mod_8", "stiles_1_mod_8", "stiles_7_mod_8", "one_tile_per_wg",
         "one_more_tile_than_wgs_on_one_xcd", "xcds_without_leftover_query_tile")


def edge_shape(edge, cus):
    """(B, N) of an order edge.  The last three are stated for the 256-query kernel (pvar 3) and derived from the CU count."""
    n_cu = (cus & ~7) // 8
    if edge == "fewer_than_8_stiles":          # 6 support tiles: ns_x = 0, everything is leftover part, no groups
        return 64 * (-(-4 * max(cus, 256) // 6)) - 44, 700
    if edge == "stiles_0_mod_8":               # no leftover part
        return 1030, BS * 8 * (-(-4 * max(cus, 256) // (17 * 8)))
    if edge == "stiles_1_mod_8":
        return 1030, BS * 8 * (-(-4 * max(cus, 256) // (17 * 8))) + 9
    if edge == "stiles_7_mod_8":
        return 1030, BS * (8 * (-(-4 * max(cus, 256) // (17 * 8))) + 7) - 120
    if edge == "one_tile_per_wg":              # 4 query tiles x CUs / 4 support tiles: n_cu tiles on each XCD's list
        assert cus % 32 == 0, f"{cus} CUs: not a multiple of 32, no shape with one 256 x 128 tile per workgroup"
        return 4 * 256, (cus // 4) * BS
    if edge == "one_more_tile_than_wgs_on_one_xcd":   # one query tile, 8 * n_cu + 1 support tiles: XCD 0 has n_cu + 1
        return 256, BS * 8 * n_cu + 100
    assert edge == "xcds_without_leftover_query_tile"  # two query tiles, n_stiles % 8 = 3: nq_x = 0 for XCDs 2..7
    return 500, BS * (8 * max(16, n_cu // 2) + 2) + 60
