"""Neighbour search over a prepared bank, three routes alternated in one process: the rounded search over an fp16 bank
(ops.nw_knn(rounded=True), nw_knn_f16), the split-row fused search (ops.nw_knn, nw_knn_f32) and the score-matrix route
(nw_scores through the split-row bank + nw_topk).  Per shape: us per search (HIP events, median of the rounds and their
spread), the workspace bytes of the two fused searches and the bytes of the score matrix, and recall@k of the rounded
search against the fp32-grade one (the share of the split-row search's rows that the rounded search returns).
  python tools/knn_half_time.py [--rounds R] [--iters I]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from nwhead_amd import _lib, ops

SHAPES = ((256, 50000, 512, 10), (256, 400000, 256, 10))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _lib.load()
    for B, N, d, k in SHAPES:
        g = torch.Generator().manual_seed(N + k)
        q = torch.randn(B, d, generator=g).to(dev)
        s = torch.randn(N, d, generator=g).to(dev)
        split, half = ops.SplitBank(s), ops.SplitBank(s, precision="fp16")

        def matrix():
            return ops.nw_topk(ops.nw_scores(q, s, "euclidean", support_cache=split), k)

        def fused():
            return ops.nw_knn(q, split, k, "euclidean", support=s)

        def rounded():
            return ops.nw_knn(q, half, k, "euclidean", rounded=True)

        exact, got = fused(), rounded()
        hit = (got[:, :, None] == exact[:, None, :]).any(dim=2).float().mean().item()
        tm, tf, tr = [], [], []
        for _ in range(args.rounds):
            tm.append(bench.time_kernel_events(matrix, args.iters, warmup=3, min_warm_ms=10) * 1e6)
            tf.append(bench.time_kernel_events(fused, args.iters, warmup=3, min_warm_ms=10) * 1e6)
            tr.append(bench.time_kernel_events(rounded, args.iters, warmup=3, min_warm_ms=10) * 1e6)
        mm, mf, mr = (statistics.median(t) for t in (tm, tf, tr))
        print(f"B={B} N={N} d={d} k={k}: rounded {mr:.1f} us [{min(tr):.1f}, {max(tr):.1f}], split-row fused {mf:.1f} us "
              f"[{min(tf):.1f}, {max(tf):.1f}], score matrix + top-k {mm:.1f} us [{min(tm):.1f}, {max(tm):.1f}]; "
              f"rounded / split-row {mr / mf:.2f}x, rounded / score matrix {mr / mm:.2f}x; workspace: rounded "
              f"{lib.nw_knn_f16_workspace_bytes(B, N, d, k) / 1e6:.1f} MB, split-row {lib.nw_knn_workspace_bytes(B, N, d, k) / 1e6:.1f} MB, "
              f"score matrix {B * N * 4 / 1e6:.1f} MB; bank bytes: fp16 {N * d * 2 / 1e6:.1f} MB, split rows {N * d * 4 / 1e6:.1f} MB; "
              f"recall@{k} of the rounded search against the split-row one: {hit:.4f}", flush=True)
        del q, s, split, half
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
