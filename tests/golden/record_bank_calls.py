"""Record what the head entry points hand to the C library over the case table of tests/bank_call_recorder.py, for
tests/test_bank_calls_gpu.py (needs the MI355X):

    python tests/golden/record_bank_calls.py <root of a checkout of the PARENT of the change under test, built> tests/golden/bank_call_records.json

The case table and the recorder are those of THIS checkout; nwhead_amd is imported from the checkout named.
bank_call_records.json was recorded from commit 8595316 (before the call resolver).  It must never be recorded from the tree
it is used to test."""
import json
import os
import sys

os.environ.setdefault("NW_SPLIT_ALWAYS", "1")        # as tests/conftest.py pins it
sys.path.insert(0, os.path.abspath(sys.argv[1]))
sys.path.insert(1, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import torch  # noqa: E402

import bank_call_recorder as R  # noqa: E402
from nwhead_amd import ops  # noqa: E402

dev = torch.device("cuda:0")
records = {}
for cid in R.case_ids():
    calls, _, raised = R.run_case(ops, dev, cid)
    records[cid] = {"calls": calls, "raises": raised}
torch.cuda.synchronize()
print(f"{len(records)} cases, {sum(len(r['calls']) for r in records.values())} calls, nwhead_amd from {os.path.dirname(ops.__file__)}")
if len(sys.argv) > 2:
    with open(sys.argv[2], "w") as f:
        json.dump(records, f, indent=1, sort_keys=True)
        f.write("\n")
