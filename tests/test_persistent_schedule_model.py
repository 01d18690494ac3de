"""The Python model of the persistent kernels' tile order (tests/persistent_schedule.py), on the CPU.

These tests check the MODEL, not the kernel: they document the order and the shapes that test_persistent_schedule_gpu.py
derives from it.  What follows the order on the device (ring slot, header buffer, vmcnt counts, the barrier pairing of a
workgroup that has no tile left) is checked there.
"""
from persistent_schedule import BS, EDGES, decode, edge_shape, n_local, workgroups


def _visits_every_tile_once(n_stiles, n_qtiles, qg):
    seen = set()
    for xcd in range(8):
        for L in range(n_local(n_stiles, n_qtiles, xcd)):
            qt, st = decode(L, xcd, n_stiles, n_qtiles, qg)
            assert 0 <= qt < n_qtiles and 0 <= st < n_stiles and (qt, st) not in seen
            seen.add((qt, st))
    assert len(seen) == n_stiles * n_qtiles, (n_stiles, n_qtiles, qg)


def test_decode_model_visits_every_tile_once():
    """Checks the Python MODEL of decode(), not the kernel: over all XCD lists every (qt, st) comes up exactly once, for
    fewer than 8 support tiles, every n_stiles % 8, n_qtiles below / at / above multiples of the group size and of 8; and
    for the tile counts of the GPU tests' shapes and of the K3 bank with a few group sizes each."""
    for n_stiles in range(1, 20):
        for n_qtiles in range(1, 20):
            for qg in (1, 2, 3, 4, 6, 8, 13, 32, 64):
                _visits_every_tile_once(n_stiles, n_qtiles, qg)
    for n_stiles, n_qtiles in ((61, 17), (61, 5), (102, 37), (102, 10), (131, 2), (257, 1), (6, 171), (71, 9), (391, 16)):
        for qg in (1, 4, 8, 13):
            _visits_every_tile_once(n_stiles, n_qtiles, qg)


def test_model_of_the_edge_shapes_on_256_cus():
    """What the order edges of test_order_edges mean on a 256-CU device, from the model."""
    cus = 256
    e = {k: edge_shape(k, cus) for k in EDGES}
    B, N = e["one_tile_per_wg"]
    assert [n_local(N // BS, B // 256, x) for x in range(8)] == [workgroups(3, cus, 0) // 8] * 8
    B, N = e["one_more_tile_than_wgs_on_one_xcd"]
    assert [n_local(-(-N // BS), -(-B // 256), x) for x in range(8)] == [33] + [32] * 7
    B, N = e["xcds_without_leftover_query_tile"]
    assert -(-N // BS) % 8 and [(-(-B // 256) - x + 7) >> 3 for x in range(8)] == [1, 1, 0, 0, 0, 0, 0, 0]
    assert -(-e["fewer_than_8_stiles"][1] // BS) < 8
    assert [-(-e[k][1] // BS) % 8 for k in ("stiles_0_mod_8", "stiles_1_mod_8", "stiles_7_mod_8")] == [0, 1, 7]
