"""Record nw_bwd_workspace_bytes / nw_bwd_uses_split of a given build of libnwhead_hip.so around every threshold of the
backward's route rule, for tests/test_backward_route_host.py:

    python tests/golden/record_bwd_workspace_bytes.py <libnwhead_hip.so of the PARENT of the change under test> tests/golden/bwd_workspace_bytes.npz

bwd_workspace_bytes.npz was recorded from the library of commit 967a252 (before plan_bwd).  It must never be recorded from
the tree it is used to test.  The shapes are stored with the answers."""
import ctypes
import itertools
import sys

import numpy as np

UNSET = -2 ** 31
Bs = [1, 15, 16, 17, 33, 256, 257]
Ns = [1, 255, 256, 257, 2047, 2048, 38300, 38301, 38304, 38305]
ds = [16, 36, 96, 992, 1000, 1024]
Cs = [0, 5, 16, 1000, 37500, 40881]
# every non-default knob state (bwd_split, bwd_no_mfma, xgemm_wgs), on a sub-grid
KNOB_STATES = [(0, UNSET, UNSET), (1, UNSET, UNSET), (UNSET, 1, UNSET), (0, 1, UNSET), (1, 1, UNSET), (UNSET, UNSET, 64),
               (1, UNSET, 1024)]
SUB = dict(Bs=[15, 16, 33, 256], Ns=[255, 256, 2048, 38300, 38305], ds=[36, 96, 1024], Cs=[5, 16, 37500])


def grid(Bs=Bs, Ns=Ns, ds=ds, Cs=Cs):
    return np.array(list(itertools.product(Bs, Ns, ds, Cs, (0, 1))), dtype=np.int64)


def answers(lib, shapes, knobs=(UNSET, UNSET, UNSET)):
    """(total bytes, uses_split) per shape under one knob state; the knobs are unset again afterwards."""
    lib.nw_bwd_workspace_bytes.restype = ctypes.c_size_t
    lib.nw_bwd_workspace_bytes.argtypes = [ctypes.c_int64] * 4 + [ctypes.c_int] * 2
    lib.nw_bwd_uses_split.restype = ctypes.c_int
    lib.nw_bwd_uses_split.argtypes = [ctypes.c_int64] * 4 + [ctypes.c_int]
    lib.nw_debug_set.argtypes = [ctypes.c_char_p, ctypes.c_int]
    names = (b"bwd_split", b"bwd_no_mfma", b"xgemm_wgs")
    for n, v in zip(names, knobs):
        assert lib.nw_debug_set(n, v) == 0
    try:
        total = np.array([lib.nw_bwd_workspace_bytes(B, N, d, C, 0, sup) for B, N, d, C, sup in shapes.tolist()], dtype=np.int64)
        split = np.array([lib.nw_bwd_uses_split(B, N, d, C, sup) for B, N, d, C, sup in shapes.tolist()], dtype=np.int8)
    finally:
        for n in names:
            lib.nw_debug_set(n, UNSET)
    return total, split


if __name__ == "__main__":
    import torch  # noqa: F401  (its HIP runtime first, as nwhead_amd._lib does)
    lib = ctypes.CDLL(sys.argv[1])
    out = {"knob_states": np.array(KNOB_STATES, dtype=np.int64), "shapes": grid(), "sub_shapes": grid(**SUB)}
    out["total"], out["split"] = answers(lib, out["shapes"])
    for i, k in enumerate(KNOB_STATES):
        out[f"total_k{i}"], out[f"split_k{i}"] = answers(lib, out["sub_shapes"], k)
    print(len(out["total"]), "shapes,", len(out["sub_shapes"]), "per knob state;", int(out["split"].sum()), "split by default")
    if len(sys.argv) > 2:
        np.savez_compressed(sys.argv[2], **out)
