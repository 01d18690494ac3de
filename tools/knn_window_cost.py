"""What the row window costs the search WITHOUT a window: nw_knn_f32 of this tree's library against the same entry of
another build of the library (the parent commit's, --parent-lib), alternated in one process on the same operands and
workspace.  Prints us per search (HIP events, median of the rounds and their spread) for both and whether the results
are bit-equal.
  python tools/knn_window_cost.py --parent-lib /path/to/libnwhead_hip.so [--rounds R] [--iters I]"""
import argparse
import ctypes
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from nwhead_amd import _lib, ops

SHAPES = ((256, 50000, 512, 10),)
ENTRIES = ("nw_knn_f32", "nw_knn_workspace_bytes", "nw_abi_version")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    here = _lib.load()
    parent = ctypes.CDLL(os.path.abspath(args.parent_lib))
    for name in ENTRIES:
        fn = getattr(parent, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    assert parent.nw_abi_version() == here.nw_abi_version()
    for B, N, d, k in SHAPES:
        g = torch.Generator().manual_seed(N + k)
        q = torch.randn(B, d, generator=g).to(dev)
        s = torch.randn(N, d, generator=g).to(dev)
        bank = ops.SplitBank(s)
        need = max(here.nw_knn_workspace_bytes(B, N, d, k), parent.nw_knn_workspace_bytes(B, N, d, k))
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        st = torch.cuda.current_stream().cuda_stream
        out = {}

        def search(lib, tag):
            idx = torch.empty(B, k, dtype=torch.int64, device=dev)
            val = torch.empty(B, k, dtype=torch.float32, device=dev)
            rc = lib.nw_knn_f32(q.data_ptr(), bank.split.data_ptr(), bank.scale.data_ptr(), bank.norm2.data_ptr(), idx.data_ptr(),
                                val.data_ptr(), ws.data_ptr(), need, B, N, d, k, 0, None, st)
            assert rc == 0, (tag, rc)
            out[tag] = (idx, val)

        search(here, "here"), search(parent, "parent")
        torch.cuda.synchronize()
        same = torch.equal(out["here"][0], out["parent"][0]) and torch.equal(out["here"][1].view(torch.int32),
                                                                             out["parent"][1].view(torch.int32))
        th, tp = [], []
        for _ in range(args.rounds):
            th.append(bench.time_kernel_events(lambda: search(here, "here"), args.iters, warmup=3, min_warm_ms=10) * 1e6)
            tp.append(bench.time_kernel_events(lambda: search(parent, "parent"), args.iters, warmup=3, min_warm_ms=10) * 1e6)
        mh, mp = statistics.median(th), statistics.median(tp)
        print(f"B={B} N={N} d={d} k={k}: nw_knn_f32 this tree {mh:.1f} us [{min(th):.1f}, {max(th):.1f}], parent library "
              f"{mp:.1f} us [{min(tp):.1f}, {max(tp):.1f}] ({mh / mp:.3f}x); bit-equal: {same}", flush=True)


if __name__ == "__main__":
    main()
