"""The head over a per-query row window of a resident bank, two routes alternated in one process:
  * fused: ops.nw_head(..., row_window=...) -> nw_fwd_window_f32, the window in the tile epilogue, no (B,N) matrix;
  * the matrix route: ops.nw_scores over the bank, a torch mask, nw_aggregate_f32 (what ops.nw_head_window falls back to);
and, for scale, the plain ops.nw_head over the same bank.
Shapes: leave-one-out over a 50000 x 512 bank of 200 classes in batches of 256 (the queries are bank rows, window
[row, row + 1) excluded), and 256 queries over 400000 x 256 with "every class but the query's own" (a class window, excluded).
Per shape: us per batch (HIP events, median of the rounds and their spread), peak extra device memory of one call of each
route (torch's allocator: outputs, masks and score matrices; the cached forward workspace is reported next to it), and how
the two answers compare.
  python tools/loo_time.py [--rounds R] [--iters I]         (NW_SPLIT_ALWAYS unset: the fused route needs no switch)"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from nwhead_amd import _lib, ops

SHAPES = (("leave-one-out", 256, 50000, 512, 200), ("other classes", 256, 400000, 256, 200))


def _peak_extra(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    del out
    return torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    args = ap.parse_args()
    if os.environ.get("NW_SPLIT_ALWAYS"):
        raise SystemExit("run with NW_SPLIT_ALWAYS unset")
    dev = torch.device("cuda:0")
    lib = _lib.load()
    for what, B, N, d, C in SHAPES:
        g = torch.Generator().manual_seed(N + d)
        s = torch.randn(N, d, generator=g).to(dev)
        sy = (torch.arange(N) % C).sort().values.to(dev)
        bank = ops.SplitBank(s, labels=sy)
        if what == "leave-one-out":
            rows = torch.randperm(N, generator=g)[:B].to(dev)
            q = s[rows].clone()
            window = (rows, rows + 1)
        else:
            q = torch.randn(B, d, generator=g).to(dev)
            qy = torch.randint(0, C, (B,), generator=g).to(dev)
            window = (torch.searchsorted(sy, qy), torch.searchsorted(sy, qy, right=True))
        lo, hi = window
        cols = torch.arange(N, device=dev)
        assert ops.head_window_route(split=bank.split is not None, sorted_copy=bank.sorted_rows is not None, shape=bank.shape,
                                     pad=bank.pad, width=d, B=B, n_classes=C) == "fused"

        def fused():
            return ops.nw_head(q, s, sy, C, support_cache=bank, row_window=window, exclude=True)

        def matrix():
            keep = ~((cols >= lo[:, None]) & (cols < hi[:, None]))
            scores = ops.nw_scores(q, s, support_cache=bank).masked_fill_(~keep, float("-inf"))
            return ops.nw_aggregate(scores, sy, C)

        def plain():
            return ops.nw_head(q, s, sy, C, support_cache=bank)

        with torch.no_grad():
            f, m = fused(), matrix()
            diff = float((f - m).abs().max())
            mem_f, mem_m = _peak_extra(fused), _peak_extra(matrix)
            tf, tm, tp = [], [], []
            for _ in range(args.rounds):
                tf.append(bench.time_kernel_events(fused, args.iters, warmup=2, min_warm_ms=10) * 1e6)
                tm.append(bench.time_kernel_events(matrix, args.iters, warmup=2, min_warm_ms=10) * 1e6)
                tp.append(bench.time_kernel_events(plain, args.iters, warmup=2, min_warm_ms=10) * 1e6)
        mf, mm, mp = (statistics.median(t) for t in (tf, tm, tp))
        print(f"{what}: B={B} N={N} d={d} C={C}: fused {mf:.1f} us [{min(tf):.1f}, {max(tf):.1f}] per batch; scores + mask + "
              f"aggregate {mm:.1f} us [{min(tm):.1f}, {max(tm):.1f}]; fused / matrix {mf / mm:.2f}x; plain nw_head over the bank "
              f"{mp:.1f} us [{min(tp):.1f}, {max(tp):.1f}]; peak extra memory fused {mem_f / 1e6:.2f} MB, matrix {mem_m / 1e6:.1f} MB "
              f"(forward workspace, cached: {lib.nw_fwd_workspace_bytes(B, N, bank.shape[1], C) / 1e6:.1f} MB); largest "
              f"|difference| of the log-probabilities {diff:.2e}"
              + (f"; the whole bank in batches of {B}: {-(-N // B)} batches, {mf * -(-N // B) / 1e3:.1f} ms fused, "
                 f"{mm * -(-N // B) / 1e3:.1f} ms matrix" if what == "leave-one-out" else ""), flush=True)
        del q, s, bank, f, m, cols
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
