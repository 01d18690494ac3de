"""The diagnostic knobs (nw_debug_set) after the eleven that nothing set were removed, on the host: the name table, and the
launch decision of the fused head (nw_debug_fwd_plan) against what the library of the commit before answered
(tests/golden/h2_fwd_plans.npz, recorded by tests/golden/record_fwd_plans.py from THAT build)."""
import ctypes
import itertools
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NW_OK, NW_ERR_INVALID_ARG = 0, -1
KNOB_UNSET = -2 ** 31
REMOVED = ("merge_mq", "merge_per_query", "merge_no_global_tables", "persistent_any_rs", "coeff_threads", "xgemm_nbuf",
           "conv_gather", "wgrad_min_stages", "wgrad_batch_wgs", "bn_inline_fin", "conv_moments_per_tile")


@pytest.fixture(scope="module")
def L():
    from nwhead_amd import _lib
    _lib.load()
    return _lib


def test_every_listed_knob_is_accepted_and_every_removed_one_refused(L):
    lib = L.load()
    assert len(L.KNOBS) == 12 and len(set(L.KNOBS)) == 12 and not set(L.KNOBS) & set(REMOVED)
    for name in L.KNOBS:   # (set to what sync_knobs last set: nothing changes)
        assert lib.nw_debug_set(name.encode(), L._knob_state.get(name, KNOB_UNSET)) == NW_OK, name
    for name in REMOVED:
        assert lib.nw_debug_set(name.encode(), 1) == NW_ERR_INVALID_ARG, name
        assert lib.nw_debug_set(name.encode(), KNOB_UNSET) == NW_ERR_INVALID_ARG, name


def test_launch_plans_are_those_of_the_library_before(L):
    lib = L.load()
    z = np.load(os.path.join(ROOT, "tests", "golden", "h2_fwd_plans.npz"))
    fields = z["fields"].tolist()
    assert fields == ["rc"] + [k for k, _ in L.FwdPlan._fields_], "nw_fwd_plan has changed: record the fixture's successor"
    want = z["plans"]
    grid = itertools.product(*(z[k].tolist() for k in ("Bs", "Ns", "ds", "forms", "outputs", "norms", "pwgs")))
    C, kind, cus = int(z["C"]), int(z["kind"]), int(z["cus"])
    n = 0
    for row, (B, N, d, form, (out, k), nrm, wg) in zip(want, grid):
        p = L.FwdPlan()
        rc = lib.nw_debug_fwd_plan(B, N, d, C, form, out, k, nrm, kind, wg, cus, ctypes.byref(p))
        got = [rc] + [getattr(p, f) for f in fields[1:]]
        assert got == row.tolist(), (B, N, d, form, out, k, nrm, wg, dict(zip(fields, zip(got, row.tolist()))))
        n += 1
    assert n == len(want) == 8 * 6 * 4 * 3 * 3 * 2 * 2
    assert want[:, fields.index("persistent")].any() and (want[:, fields.index("status")] != NW_OK).any()


def test_forced_tile_heights_other_than_128_rows_are_never_persistent(L):
    lib = L.load()
    assert L.fwd_plan(2048, 50000, 512, 200, cus=256).persistent
    try:
        for rs in (6, 10, 12):
            assert lib.nw_debug_set(b"tile_rs", rs) == NW_OK
            p = L.fwd_plan(2048, 50000, 512, 200, cus=256)
            assert (p.status, p.rs, p.persistent, p.run_tables, p.variant, p.workgroups) == (NW_OK, rs, 0, 0, 0, 0)
    finally:
        assert lib.nw_debug_set(b"tile_rs", L._knob_state.get("tile_rs", KNOB_UNSET)) == NW_OK   # what sync_knobs last set
    assert L.fwd_plan(2048, 50000, 512, 200, cus=256).persistent
