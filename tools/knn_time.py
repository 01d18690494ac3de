"""Neighbour search over a prepared bank: the score-matrix route (nw_scores through the bank + nw_topk) against the fused
search (ops.nw_knn, no (B,N) matrix), alternated in one process.  Per shape: us per search (HIP events, median of the
rounds and their spread), the bytes of the score matrix and of the fused search's workspace, and whether the rows agree.
  python tools/knn_time.py [--rounds R] [--iters I] [--trace]     (--trace: a few calls of each route only, for a
  kernel-trace run: the per-kernel split is read from the profiler's statistics)"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from nwhead_amd import _lib, ops

SHAPES = ((256, 10000, 512, 10), (256, 50000, 512, 10), (256, 50000, 512, 32), (256, 400000, 256, 10))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _lib.load()
    for B, N, d, k in SHAPES:
        g = torch.Generator().manual_seed(N + k)
        q = torch.randn(B, d, generator=g).to(dev)
        s = torch.randn(N, d, generator=g).to(dev)
        bank = ops.SplitBank(s)

        def parent():
            return ops.nw_topk(ops.nw_scores(q, s, "euclidean", support_cache=bank), k)

        def fused():
            return ops.nw_knn(q, bank, k, "euclidean", support=s)

        same = torch.equal(parent(), fused())
        if args.trace:
            for _ in range(3):
                parent()
                fused()
            torch.cuda.synchronize()
            continue
        tp, tf = [], []
        for _ in range(args.rounds):
            tp.append(bench.time_kernel_events(parent, args.iters, warmup=3, min_warm_ms=10) * 1e6)
            tf.append(bench.time_kernel_events(fused, args.iters, warmup=3, min_warm_ms=10) * 1e6)
        mp, mf = statistics.median(tp), statistics.median(tf)
        print(f"B={B} N={N} d={d} k={k}: score matrix + top-k {mp:.1f} us [{min(tp):.1f}, {max(tp):.1f}], "
              f"fused {mf:.1f} us [{min(tf):.1f}, {max(tf):.1f}] ({mf / mp:.2f}x); "
              f"score matrix {B * N * 4 / 1e6:.1f} MB, fused workspace {lib.nw_knn_workspace_bytes(B, N, d, k) / 1e6:.1f} MB; "
              f"rows equal: {same}", flush=True)
        del q, s, bank
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
