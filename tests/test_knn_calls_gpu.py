"""The routes of the neighbour-search callers -- ops.nw_knn, KNN.indices, NWNet.get_neighbors, ShardedBank -- case by case
against the records of the parent of the change that gave them one route rule (tests/golden/knn_call_records.json, written by
tests/golden/record_knn_calls.py from commit 2b490eb -- never from the tree under test): the library entries every case of
tests/knn_call_recorder.py calls, their scalars, pointer roles, workspace sizes and options, the exception raised, and the
rows and value bits returned."""
import json
import os

import pytest
import torch

import knn_call_recorder as K

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def golden_records():
    with open(os.path.join(HERE, "golden", "knn_call_records.json")) as f:
        return json.load(f)


def _entries(rec):
    return [c["entry"] for c in rec["calls"]]


def test_records_cover_every_route(golden_records):
    """(no GPU: the golden file alone)  Every route and both error types occur in the parent's records."""
    assert sorted(golden_records) == sorted(K.case_ids())
    recs = list(golden_records.values())
    for entry in ("nw_knn_f32", "nw_knn_window_f32", "nw_knn_f16"):
        assert any(entry in _entries(r) for r in recs), entry
    score_calls = ("nw_fwd_f32", "nw_scores_f32")
    assert any(a in score_calls and b == "nw_topk_f32" for r in recs for a, b in zip(_entries(r), _entries(r)[1:]))
    for err in ("NWHipError", "ValueError"):
        assert any((r["raises"] or "").startswith(err + ": ") for r in recs), err


@pytest.mark.gpu
@pytest.mark.parametrize("bank", list(K.BANKS))
def test_routes_match_parent(golden_records, bank):
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    from nwhead_amd import ops
    cases = [c for c in K.case_ids() if c.split("/")[0] == bank]
    assert cases
    for cid in cases:
        got, want = K.run_case(ops, torch.device("cuda:0"), cid), golden_records[cid]
        assert got["raises"] == want["raises"], cid
        assert _entries(got) == _entries(want), cid
        for a, b in zip(got["calls"], want["calls"]):
            assert a == b, (cid, a["entry"])
        assert got["out"] == want["out"], cid
