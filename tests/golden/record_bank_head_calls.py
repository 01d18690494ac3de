"""Record what the callers of the head over a resident bank hand the library, over the case table of
tests/bank_head_call_recorder.py, for tests/test_bank_head_calls_gpu.py (needs the MI355X):

    python tests/golden/record_bank_head_calls.py <root of a checkout of the PARENT of the change under test, built> tests/golden/bank_head_call_records.json

The case table and the recorder are those of THIS checkout; nwhead_amd is imported from the checkout named, through its
public callers only.  bank_head_call_records.json was recorded from commit 967816f (before the one argument rule, route
rule and launch path of the bank head).  It must never be recorded from the tree it is used to test."""
import json
import os
import sys

os.environ.setdefault("NW_SPLIT_ALWAYS", "1")        # as tests/conftest.py pins it
sys.path.insert(0, os.path.abspath(sys.argv[1]))
sys.path.insert(1, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import torch  # noqa: E402

import bank_head_call_recorder as H  # noqa: E402
from nwhead_amd import ops  # noqa: E402

dev = torch.device("cuda:0")
records = {cid: H.run_case(ops, dev, cid) for cid in H.case_ids()}
torch.cuda.synchronize()
print(f"{len(records)} cases, {sum(len(r['calls']) for r in records.values())} calls, "
      f"{sum(r['raises'] is not None for r in records.values())} raise, nwhead_amd from {os.path.dirname(ops.__file__)}")
if len(sys.argv) > 2:
    with open(sys.argv[2], "w") as f:
        json.dump(records, f, indent=None, sort_keys=True, separators=(",", ":"))
        f.write("\n")
