"""What the head entry points hand to the C library, call by call, against the records of the parent of the change that
introduced ops._resolve (tests/golden/bank_call_records.json, written by tests/golden/record_bank_calls.py from commit
8595316 -- never from the tree under test): which rows, labels, norms, operand tensors, query width, workspace size and
nw_fwd_opts every (bank, call) pair of tests/bank_call_recorder.py resolves to, and the errors the argument checks raise."""
import json
import os

import pytest
import torch

import bank_call_recorder as R

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from nwhead_amd import ops
    return ops


@pytest.fixture(scope="module")
def golden_records():
    with open(os.path.join(HERE, "golden", "bank_call_records.json")) as f:
        return json.load(f)


def test_case_table_is_the_recorded_one(golden_records):
    assert sorted(golden_records) == sorted(R.case_ids())


@pytest.mark.parametrize("bank", list(R.BANKS) + ["none_d257"])
def test_library_calls_match_parent(dev, ops, golden_records, bank):
    cases = [c for c in R.case_ids() if c.split("/")[0] == bank]
    assert cases
    for cid in cases:
        calls, outs, raised = R.run_case(ops, dev, cid)
        want = golden_records[cid]
        assert raised == want["raises"], cid
        assert len(calls) == len(want["calls"]), (cid, [c["entry"] for c in calls])
        for got, ref in zip(calls, want["calls"]):
            assert got == ref, (cid, got["entry"])
        assert raised is not None or all(torch.isfinite(o).all() for o in outs if o.is_floating_point()), cid


def test_training_step_case_takes_both_width_rules(golden_records):
    """The recorded training step is one where the d % 4 and the d % 32 rule fired: 257 -> 260 -> 288 columns, rows split."""
    split, fwd = golden_records["none_d257/train_step"]["calls"]
    assert split["entry"] == "nw_split_rows_f16x2" and split["scalars"]["d"] == 288
    assert fwd["scalars"]["d"] == 288 and fwd["pointers"]["operand"] == "other" and fwd["pointers"]["scores"] == "other"


# ---- the argument checks: exception types and texts of the parent
def _bank_inputs(ops, dev, name):
    return R._inputs(ops, dev, name)


def test_error_n_classes_not_above_label_max(dev, ops):
    q, s, sy, bank = _bank_inputs(ops, dev, "f32_sorted")
    with pytest.raises(ValueError, match=r"support label 4 is outside \[0, n_classes=4\) \(the reference's F\.one_hot, nw\.py:276, raises\)"):
        ops.nw_head(q, s, sy, 4, support_cache=bank)
    with pytest.raises(ValueError, match=r"support label 4 is outside \[0, n_classes=3\) \(the reference's F\.one_hot, nw\.py:276, raises\)"):
        ops.nw_partials(q, s, sy, 3, support_cache=bank)         # (through the run tables' own bound)


def test_error_negative_label_at_construction(dev, ops):
    q, s, sy, _ = _bank_inputs(ops, dev, "f32_sorted")
    bad = sy.clone()
    bad[0] = -1
    msg = r"support labels must be non-negative class indices \(F\.one_hot, nw\.py:276, raises too\)"
    with pytest.raises(ValueError, match=msg):
        ops.SplitBank(s, labels=bad)
    with pytest.raises(ValueError, match=msg):
        ops.SplitBank(s).build_tables(bad)


def test_error_validate_labels(dev, ops):
    q, s, sy, _ = _bank_inputs(ops, dev, "none_d64")
    with pytest.raises(RuntimeError, match=r"^Class values must be smaller than num_classes\.$"):
        ops.nw_head(q, s, sy, R.C - 1, validate_labels=True)
    bad = sy.clone()
    bad[0] = -1
    with pytest.raises(RuntimeError, match=r"^Class values must be non-negative\.$"):
        ops.nw_head(q, s, bad, R.C, validate_labels=True)


def test_error_query_width_against_fp16_bank(dev, ops):
    q, s, sy, bank = _bank_inputs(ops, dev, "f16_sorted")
    with pytest.raises(ValueError, match=r"queries of width 100 against an fp16 bank of \(padded\) width 192"):
        ops.nw_head(q[:, :100].contiguous(), s, sy, R.C, support_cache=bank)


def test_error_bank_of_another_tensor(dev, ops):
    q, s, sy, bank = _bank_inputs(ops, dev, "f32_sorted")
    with pytest.raises(ValueError, match=r"support_cache was prepared from another support tensor \(or the tensor was modified "
                                         r"in place since\): build a new ops\.SplitBank\(s\)"):
        ops.nw_head(q, s.clone(), sy, R.C, support_cache=bank)
    with pytest.raises(ValueError, match=r"^support_cache was prepared from another support tensor$"):
        ops.nw_head_influence(q, s.clone(), sy, R.C, torch.zeros(R.B, dtype=torch.int64, device=dev), support_cache=bank)
