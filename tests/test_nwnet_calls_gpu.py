"""What the public entry points of NWNet -- precompute, predict in its six modes, predict_loo, forward_bank, refresh_bank,
get_neighbors, explain, set_support_weights -- hand the library after precompute(), after precompute_sharded() and after
both, case by case against the records of the parent of the change that gave NWNet one bank-state rule, one bank getter and
one routed neighbour search (tests/golden/nwnet_call_records.json, written by tests/golden/record_nwnet_calls.py from commit
2486763 -- never from the tree under test): the library entries every case of tests/nwnet_call_recorder.py calls, their
scalars, pointer roles and workspace sizes, the exception raised, the bits of the results and gradients, and the state the
call leaves (full_cache rebuilt or not, bank_features, the support_logw parameter, the (out, mask) pair)."""
import json
import os

import pytest
import torch

import nwnet_call_recorder as W

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def golden_records():
    with open(os.path.join(HERE, "golden", "nwnet_call_records.json")) as f:
        return json.load(f)


def _entries(rec):
    return [c["entry"] for c in rec["calls"]]


def test_records_cover_every_entry_point_and_route(golden_records):
    """(no GPU: the golden file alone)  Every entry point in every bank state, the three routes of the neighbour search, the
    weighted head with its weights' gradient, the row update and both error types occur in the parent's records."""
    assert sorted(golden_records) == sorted(W.case_ids())
    for state in W.STATES:
        for entry in ("precompute", "predict-", "predict_loo", "forward_bank", "refresh_bank", "get_neighbors", "explain",
                      "set_support_weights"):
            assert any(cid.startswith(f"d64_N40/{state}/{entry}") for cid in golden_records), (state, entry)
    for mode in ("random", "full", "cluster", "ensemble", "knn", "hnsw"):
        assert golden_records[f"d64_N40/resident/predict-{mode}"]["raises"] is None, mode
    recs = list(golden_records.values())
    neighbors = [r for cid, r in golden_records.items() if "/get_neighbors-" in cid]
    # the fused search, the rounded search, and the score matrix ranked by nw_knn
    for entry in ("nw_knn_f32", "nw_knn_f16", "nw_topk_f32"):
        assert any(entry in _entries(r) for r in neighbors), entry
    for entry in ("nw_fwd_weighted_f32", "nw_fwd_window_f32", "nw_bwd_query_logw_f32", "nw_bwd_query_weighted_f32",
                  "nw_bank_update_rows_f32", "nw_influence_select_f32", "nw_knn_merge_f32", "nw_split_rows_f16x2"):
        assert any(entry in _entries(r) for r in recs), entry
    for err in ("NWHipError", "ValueError"):
        assert any((r["raises"] or "").startswith(err + ": ") for r in recs), err
    for flag in ("rebuilt", "bank_features", "logw_parameter", "pair"):
        assert any(r["state"][flag] for r in recs) and not all(r["state"][flag] for r in recs), flag


@pytest.mark.gpu
@pytest.mark.parametrize("net", list(W.NETS))
def test_calls_match_parent(golden_records, net):
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    import nwhead_amd
    cases = W.case_ids(net)
    assert cases
    for cid in cases:
        got, want = W.run_case(nwhead_amd, cid), golden_records[cid]
        assert got["raises"] == want["raises"], cid
        assert _entries(got) == _entries(want), cid
        for a, b in zip(got["calls"], want["calls"]):
            assert a == b, (cid, a["entry"])
        assert got["state"] == want["state"], cid
        assert got["out"] == want["out"], cid
