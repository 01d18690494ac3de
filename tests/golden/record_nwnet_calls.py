"""Record what the public entry points of NWNet hand the library in every bank state, over the case table of
tests/nwnet_call_recorder.py, for tests/test_nwnet_calls_gpu.py (needs the MI355X):

    python tests/golden/record_nwnet_calls.py <root of a checkout of the PARENT of the change under test, built> tests/golden/nwnet_call_records.json

The case table and the recorder are those of THIS checkout; nwhead_amd is imported from the checkout named, through its
public methods only.  nwnet_call_records.json was recorded from commit 2486763 (before NWNet's one bank-state rule, one bank
getter and one routed neighbour search).  It must never be recorded from the tree it is used to test."""
import json
import os
import sys

os.environ.setdefault("NW_SPLIT_ALWAYS", "1")        # as tests/conftest.py pins it
sys.path.insert(0, os.path.abspath(sys.argv[1]))
sys.path.insert(1, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import torch  # noqa: E402

import nwhead_amd  # noqa: E402
import nwnet_call_recorder as W  # noqa: E402
from nwhead_amd import ops  # noqa: E402,F401

records = {cid: W.run_case(nwhead_amd, cid) for cid in W.case_ids()}
torch.cuda.synchronize()
print(f"{len(records)} cases, {sum(len(r['calls']) for r in records.values())} calls, "
      f"{sum(r['raises'] is not None for r in records.values())} raise, nwhead_amd from {os.path.dirname(nwhead_amd.__file__)}")
if len(sys.argv) > 2:
    with open(sys.argv[2], "w") as f:
        json.dump(records, f, indent=None, sort_keys=True, separators=(",", ":"))
        f.write("\n")
