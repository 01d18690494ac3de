"""What the callers of the head over a resident bank -- ops.nw_head(row_window=... / row_logw=...), ops.nw_head_window,
ops.nw_head_bank -- hand the library, case by case against the records of the parent of the change that gave them one
regime, one forward launch and one backward launch (tests/golden/bank_head_call_records.json, written by
tests/golden/record_bank_head_calls.py from commit 967816f -- never from the tree under test): the library entries every
case of tests/bank_head_call_recorder.py calls, their scalars, pointer roles and workspace sizes, the exception raised, and
the bits of the results and gradients (forward and backward are reproducible: no float atomics)."""
import json
import os

import pytest
import torch

import bank_head_call_recorder as H

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def golden_records():
    with open(os.path.join(HERE, "golden", "bank_head_call_records.json")) as f:
        return json.load(f)


def _entries(rec):
    return [c["entry"] for c in rec["calls"]]


def test_records_cover_every_route(golden_records):
    """(no GPU: the golden file alone)  Every entry, every fallback and both error types occur in the parent's records."""
    assert sorted(golden_records) == sorted(H.case_ids())
    recs = list(golden_records.values())
    for entry in ("nw_fwd_window_f32", "nw_fwd_weighted_f32", "nw_bwd_query_f32", "nw_bwd_query_weighted_f32",
                  "nw_bwd_query_logw_f32", "nw_bwd_query_workspace_bytes", "nw_bwd_logw_workspace_bytes", "nw_fwd_f32"):
        assert any(entry in _entries(r) for r in recs), entry
    assert any(a == "nw_scores_f32" and b == "nw_aggregate_f32" for r in recs for a, b in zip(_entries(r), _entries(r)[1:]))
    # the no-window forward of nw_head_bank: nw_fwd_f32, then the query gradient over the bank
    assert any(a == "nw_fwd_f32" and b == "nw_bwd_query_workspace_bytes" for r in recs for a, b in zip(_entries(r), _entries(r)[1:]))
    # the weights' gradient with and without the queries'
    want_gq = {c["scalars"]["want_gq"] for r in recs for c in r["calls"] if c["entry"] == "nw_bwd_logw_workspace_bytes"}
    assert want_gq == {0, 1}
    assert any(c["pointers"]["gq"] is None for r in recs for c in r["calls"] if c["entry"] == "nw_bwd_query_logw_f32")
    for err in ("NWHipError", "ValueError"):
        assert any((r["raises"] or "").startswith(err + ": ") for r in recs), err


@pytest.mark.gpu
@pytest.mark.parametrize("bank", list(H.BANKS))
def test_calls_match_parent(golden_records, bank):
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    from nwhead_amd import ops
    cases = H.case_ids(bank)
    assert cases
    for cid in cases:
        got, want = H.run_case(ops, torch.device("cuda:0"), cid), golden_records[cid]
        assert got["raises"] == want["raises"], cid
        assert _entries(got) == _entries(want), cid
        for a, b in zip(got["calls"], want["calls"]):
            assert a == b, (cid, a["entry"])
        assert got["out"] == want["out"], cid
