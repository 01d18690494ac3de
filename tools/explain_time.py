"""The k most helpful and most harmful supports of every query, two routes alternated in one process:
  * ops.nw_top_influence: one forward, two windowed searches over the class-sorted bank (nw_knn_window_f32), two
    nw_influence_select_f32 launches -- no (B,N) matrix;
  * the matrix route: ops.nw_head_influence, then two masked torch.topk over the (B,N) influence matrix.
Per shape: us per call (HIP events, median of the rounds and their spread), the share of the two searches in the new
route, the bytes of the influence matrix and its masks against the search workspace, and how the two answers compare.
  python tools/explain_time.py [--rounds R] [--iters I]         (NW_SPLIT_ALWAYS unset: both shapes are fused on their own)"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from nwhead_amd import _lib, ops

SHAPES = ((256, 50000, 512, 200, 10), (256, 400000, 256, 200, 10))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    args = ap.parse_args()
    if os.environ.get("NW_SPLIT_ALWAYS"):
        raise SystemExit("run with NW_SPLIT_ALWAYS unset")
    dev = torch.device("cuda:0")
    lib = _lib.load()
    for B, N, d, C, k in SHAPES:
        g = torch.Generator().manual_seed(N + k)
        q = torch.randn(B, d, generator=g).to(dev)
        s = torch.randn(N, d, generator=g).to(dev)
        sy = (torch.arange(N) % C).sort().values.to(dev)
        qy = torch.randint(0, C, (B,), generator=g).to(dev)
        bank = ops.SplitBank(s, labels=sy)
        same = sy[None, :] == qy[:, None]
        window = (torch.searchsorted(sy, qy), torch.searchsorted(sy, qy, right=True))

        def new():
            return ops.nw_top_influence(q, s, sy, C, qy, k, support_cache=bank)

        def searches():
            return (ops.nw_knn(q, bank, k, return_values=True, support=s, row_window=window),
                    ops.nw_knn(q, bank, k, return_values=True, support=s, row_window=window, exclude=True))

        def matrix():
            out, infl = ops.nw_head_influence(q, s, sy, C, qy, support_cache=bank)
            helpful = torch.topk(infl.masked_fill(~same, float("-inf")), k, dim=1)
            harmful = torch.topk(infl.masked_fill(same, float("inf")), k, dim=1, largest=False)
            return out, helpful, harmful

        r, m = new(), matrix()
        # The matrix route ranks influences, the new one scores.  Where the softmax is peaked most influences round to +-0
        # in the matrix and its top-k breaks those ties as it likes: rows are compared where the influence is not zero.
        got_v, ref_v = torch.cat([r.helpful_infl, r.harmful_infl], 1), torch.cat([m[1].values, m[2].values], 1)
        got_r, ref_r = torch.cat([r.helpful_rows, r.harmful_rows], 1), torch.cat([m[1].indices, m[2].indices], 1)
        live = (ref_v != 0) & torch.isfinite(ref_v)
        vdiff = float((got_v - ref_v)[torch.isfinite(ref_v)].abs().max())
        agree = torch.equal(got_r[live], ref_r[live])
        tn, ts, tm = [], [], []
        for _ in range(args.rounds):
            tn.append(bench.time_kernel_events(new, args.iters, warmup=2, min_warm_ms=10) * 1e6)
            ts.append(bench.time_kernel_events(searches, args.iters, warmup=2, min_warm_ms=10) * 1e6)
            tm.append(bench.time_kernel_events(matrix, args.iters, warmup=2, min_warm_ms=10) * 1e6)
        mn, ms, mm = (statistics.median(t) for t in (tn, ts, tm))
        dp = bank.shape[1]
        print(f"B={B} N={N} d={d} C={C} k={k}: nw_top_influence {mn:.1f} us [{min(tn):.1f}, {max(tn):.1f}], of which the two "
              f"windowed searches {ms:.1f} us [{min(ts):.1f}, {max(ts):.1f}] ({ms / mn:.2f} of it); nw_head_influence + two "
              f"masked topk {mm:.1f} us [{min(tm):.1f}, {max(tm):.1f}]; new / matrix {mn / mm:.2f}x; influence matrix "
              f"{B * N * 4 / 1e6:.1f} MB + masks and masked copies {B * N * (1 + 2 * 4) / 1e6:.1f} MB, search workspace "
              f"{lib.nw_knn_workspace_bytes(B, N, dp, k) / 1e6:.1f} MB; largest |difference| of the 2k influence values per query "
              f"{vdiff:.2e}; rows equal where the matrix route's influence is not +-0 ({float(live.float().mean()):.2f} of the "
              f"entries): {agree}", flush=True)
        del q, s, bank, same, r, m
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
