"""Record every field of nw_debug_fwd_plan's answer of a given build of libnwhead_hip.so over a grid of calls, for
tests/test_knobs_host.py:

    python tests/golden/record_fwd_plans.py <libnwhead_hip.so of the PARENT of the change under test> tests/golden/h2_fwd_plans.npz

h2_fwd_plans.npz was recorded from the library of commit 6899865 (before the eleven unused diagnostic knobs were removed).
It must never be recorded from the tree it is used to test."""
import ctypes
import itertools
import sys

import numpy as np
import torch  # noqa: F401  (its HIP runtime first, as nwhead_amd._lib does)

FIELDS = ("status", "rs", "bs", "n_stiles", "n_qtiles", "grid", "mode", "out", "dma", "persistent", "variant", "workgroups",
          "qgroup", "split_queries", "run_tables", "reserved")


class FwdPlan(ctypes.Structure):   # nw_fwd_plan (include/nwhead_hip.h)
    _fields_ = [(k, ctypes.c_int32) for k in FIELDS] + [("lds_bytes", ctypes.c_uint64)]


Bs = [1, 64, 130, 256, 384, 512, 2048, 6656]
Ns = [26, 400, 2100, 10000, 50000, 400000]
ds = [32, 36, 96, 512]
forms = [0, 1, 2]                      # fp32, split, half
outputs = [(0, 0), (1, 0), (2, 10)]    # (log_probs, scores, candidates) x k
norms = [1, 0]
pwgs = [0, 248]
C, KIND, CUS = 200, 0, 256


def record(lib):
    """(calls, 1 + len(FIELDS) + 1) int64: the call's return value, then the plan's fields, in the order of the lists above."""
    f = lib.nw_debug_fwd_plan
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_int64] * 4 + [ctypes.c_int] * 7 + [ctypes.c_void_p]
    rows = []
    for B, N, d, form, (out, k), nrm, wg in itertools.product(Bs, Ns, ds, forms, outputs, norms, pwgs):
        p = FwdPlan()
        rc = f(B, N, d, C, form, out, k, nrm, KIND, wg, CUS, ctypes.byref(p))
        rows.append([rc] + [getattr(p, k_) for k_ in FIELDS] + [p.lds_bytes])
    return np.array(rows, dtype=np.int64)


if __name__ == "__main__":
    plans = record(ctypes.CDLL(sys.argv[1]))
    if len(sys.argv) > 2:
        np.savez_compressed(sys.argv[2], Bs=np.array(Bs), Ns=np.array(Ns), ds=np.array(ds), forms=np.array(forms),
                            outputs=np.array(outputs), norms=np.array(norms), pwgs=np.array(pwgs), C=np.array(C),
                            kind=np.array(KIND), cus=np.array(CUS), fields=np.array(("rc",) + FIELDS + ("lds_bytes",)),
                            plans=plans)
