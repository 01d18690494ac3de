"""Which bank serves every public entry point of NWNet in every bank state, and what it refuses with (nw.bank_rule), cell by
cell against the records of the parent of the change that gave NWNet one bank-state rule, one bank getter and one routed
neighbour search (tests/golden/nwnet_rules.json, written by tests/golden/record_nwnet_rules.py from commit 2486763 -- never from
the tree under test): the exception, the stubbed ops calls in order with their distinguishing keywords, and the state the
call leaves.  No device: the ops functions are stubs."""
import importlib.util
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def _recorder():
    spec = importlib.util.spec_from_file_location("record_nwnet_rules", os.path.join(HERE, "golden", "record_nwnet_rules.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def golden_table():
    with open(os.path.join(HERE, "golden", "nwnet_rules.json")) as f:
        return _recorder().unpack(json.load(f))      # (every distinct record once, and the index of every cell's)


def test_table_covers_every_state_mode_and_error(golden_table):
    """(the golden file alone)"""
    R = _recorder()
    assert sorted(golden_table) == sorted(R.cell_ids())
    assert {cid[:4] for cid in golden_table} >= {f"r{r}s{s}" for r in "01" for s in "01"}          # the four bank states
    for mode in R.MODES:
        assert any(f"/predict-{mode}" in cid and rec["raises"] is None for cid, rec in golden_table.items()), mode
    for err in ("NWHipError", "ValueError"):
        assert any((rec["raises"] or "").startswith(err + ": ") for rec in golden_table.values()), err
    calls = {c.split("(")[0] for rec in golden_table.values() for c in rec["calls"]}
    assert calls >= {"SplitBank", "SplitBank.update_rows", "nw_head", "nw_head_bank", "nw_scores", "nw_topk", "nw_top_influence",
                     "nw_aggregate", "sharded.predict", "sharded.predict_knn", "sharded.neighbors"}
    assert any(rec["rebuilt"] for rec in golden_table.values()) and any(rec["pair"] for rec in golden_table.values())
    assert any("row_logw=parameter" in c for rec in golden_table.values() for c in rec["calls"])


def test_tree_reproduces_the_parent_cell_for_cell(golden_table):
    R = _recorder()
    for cid in R.cell_ids():
        assert R.run_cell(cid) == golden_table[cid], cid


def test_bank_rule_agrees_with_the_parent_over_the_grid(golden_table):
    """The pure rule against what the parent DID: a Refusal is the recorded exception to the letter, "missing" an
    AttributeError, "sharded" a call of the sharded bank first; "resident" and "supports" raise nothing and leave the sharded
    bank alone."""
    from nwhead_amd.nwhead.nw import Refusal, bank_rule
    R = _recorder()
    asked = 0
    for cid in R.cell_ids():
        if cid in R.EXTRA_IDS or cid.endswith("/set_support_weights-none"):      # argument errors; clearing asks nothing
            continue
        entry, kw = R.facts(cid)
        served = bank_rule(entry, "forward_bank" if entry == "weights_for" else None, **kw)
        rec = golden_table[cid]
        asked += 1
        if isinstance(served, Refusal):
            assert rec["raises"] == f"{served.kind.__name__}: {served.text}", cid
            if served.early:            # before any work: no stub was reached, nothing was kept
                assert rec["calls"] == [] and not rec["bank_features"], cid
        elif served == "missing":
            assert rec["raises"].startswith("AttributeError: "), cid
        else:
            assert rec["raises"] is None, cid
            assert served in ("resident", "sharded", "supports"), cid
            assert any(c.startswith("sharded.") for c in rec["calls"]) == (served == "sharded"), cid
    assert asked == len(R.STATES) * len(R.NETS) * (len(R.CALLS) - 1)
