"""Record nw_knn_workspace_bytes / nw_fwd_workspace_bytes of a given build of libnwhead_hip.so over the grids of
tests/test_knn_fused_host.py, for tests/test_launch_plan_host.py:

    python tests/golden/record_workspace_bytes.py <libnwhead_hip.so of the PARENT of the change under test> tests/golden/h1_workspace_bytes.npz

h1_workspace_bytes.npz was recorded from the library of commit 26200c0 (before the launch plan).  It must never be recorded
from the tree it is used to test."""
import ctypes
import sys

import numpy as np
import torch  # noqa: F401  (its HIP runtime first, as nwhead_amd._lib does)

lib = ctypes.CDLL(sys.argv[1])
for n in ("nw_knn_workspace_bytes", "nw_fwd_workspace_bytes"):
    f = getattr(lib, n)
    f.restype = ctypes.c_size_t
    f.argtypes = [ctypes.c_int64] * 4
Ns = [26, 27, 32, 33, 100, 400, 1000, 1001, 1999, 2000, 2100, 4100, 8000, 10000, 16000, 20000, 32000, 33000, 50000, 400000]
Bs = [1, 37, 64, 65, 130, 200, 256, 257, 512, 1000, 4096]
ks = [1, 4, 5, 10, 20, 32]
ds = [32, 512]
C = 200
knn = np.array([[[[lib.nw_knn_workspace_bytes(B, N, d, k) for k in ks] for N in Ns] for B in Bs] for d in ds], dtype=np.int64)
fwd = np.array([[[lib.nw_fwd_workspace_bytes(B, N, d, C) for N in Ns] for B in Bs] for d in ds], dtype=np.int64)
stretch = np.array([lib.nw_knn_workspace_bytes(256, N, 512, 10) for N in range(1900, 2300)], dtype=np.int64)
if len(sys.argv) > 2:
    np.savez_compressed(sys.argv[2], Ns=np.array(Ns), Bs=np.array(Bs), ks=np.array(ks), ds=np.array(ds), C=np.array(C),
                        knn=knn, fwd=fwd, stretch_N0=np.array(1900), stretch=stretch)
