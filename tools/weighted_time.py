"""The head with support weights (a log-weight per bank row) over a resident bank, four routes alternated in one process:
  * weighted: ops.nw_head(..., row_logw=a) -> nw_fwd_weighted_f32, the weight added in the tile epilogue, no (B,N) matrix;
  * windowed: ops.nw_head(..., row_window=whole bank) -> nw_fwd_window_f32, the same kernel minus the weight: the floor the
    weighted route should sit near (it reads N more floats per query tile);
  * plain:    ops.nw_head over the same bank (the persistent kernels where the shape has them);
  * matrix:   ops.nw_scores over the bank + a + nw_aggregate_f32, what the weighted head falls back to, with its (B,N) matrix;
and forward + backward in the queries for the same routes (ops.nw_head_bank: nw_bwd_query_weighted_f32, nw_bwd_query_f32
with and without the whole-bank window).  The library has no gradient route through the score matrix that knows the weights
(head_weighted_route): nw_head's route through the score matrix, WITHOUT weights, stands in the fourth place as what such
a route would cost at the least.
Weights: a_j by j mod 7 = {0, ln 2, -3.5, -inf, 0, 1.25, -0.5}.
Per shape: us per call (HIP events, median of the rounds and their spread), the peak extra device memory of one call of each
forward route, and how the weighted answers of the fused and the matrix route compare.
  python tools/weighted_time.py [--rounds R] [--iters I]         (NW_SPLIT_ALWAYS unset)"""
import argparse
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from nwhead_amd import ops

SHAPES = ((256, 50000, 512, 200), (256, 400000, 256, 200))
PATTERN = (0.0, math.log(2.0), -3.5, float("-inf"), 0.0, 1.25, -0.5)


def _peak_extra(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    del out
    return torch.cuda.max_memory_allocated() - base


def _fmt(name, t):
    return f"{name} {statistics.median(t):.1f} us [{min(t):.1f}, {max(t):.1f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    args = ap.parse_args()
    if os.environ.get("NW_SPLIT_ALWAYS"):
        raise SystemExit("run with NW_SPLIT_ALWAYS unset")
    dev = torch.device("cuda:0")
    for B, N, d, C in SHAPES:
        g = torch.Generator().manual_seed(N + d)
        s = torch.randn(N, d, generator=g).to(dev)
        sy = (torch.arange(N) % C).sort().values.to(dev)
        bank = ops.SplitBank(s, labels=sy)
        q = torch.randn(B, d, generator=g).to(dev)
        a = torch.tensor(PATTERN)[torch.arange(N) % 7].to(dev)
        gout = torch.randn(B, C, generator=g).to(dev)
        whole = (torch.zeros(B, dtype=torch.int64, device=dev), torch.full((B,), N, device=dev))
        facts = dict(split=bank.split is not None, sorted_copy=bank.sorted_rows is not None, shape=bank.shape, pad=bank.pad,
                     width=d, B=B, n_classes=C)
        assert ops.head_weighted_route(**facts) == "fused" and ops.head_weighted_route(**facts, grad=True) == "fused"

        fwd = {
            "weighted": lambda: ops.nw_head(q, s, sy, C, support_cache=bank, row_logw=a),
            "windowed": lambda: ops.nw_head(q, s, sy, C, support_cache=bank, row_window=whole),
            "plain": lambda: ops.nw_head(q, s, sy, C, support_cache=bank),
            "matrix": lambda: ops.nw_aggregate(ops.nw_scores(q, s, support_cache=bank).add_(a), sy, C),
        }

        def step(head):
            def run():
                qg = q.detach().requires_grad_(True)
                head(qg).backward(gout)
                return qg.grad
            return run

        bwd = {
            "weighted": step(lambda qg: ops.nw_head_bank(qg, s, sy, C, bank, row_logw=a)),
            "windowed": step(lambda qg: ops.nw_head_bank(qg, s, sy, C, bank, row_window=whole)),
            "plain": step(lambda qg: ops.nw_head_bank(qg, s, sy, C, bank)),
            "nw_head through the score matrix (no weights)": step(lambda qg: ops.nw_head(qg, s, sy, C, support_cache=bank)),
        }
        with torch.no_grad():
            diff = float((fwd["weighted"]() - fwd["matrix"]()).abs().max())
            mem = {k: _peak_extra(f) for k, f in fwd.items()}
            tf = {k: [] for k in fwd}
            for _ in range(args.rounds):
                for k, f in fwd.items():
                    tf[k].append(bench.time_kernel_events(f, args.iters, warmup=2, min_warm_ms=10) * 1e6)
        tb = {k: [] for k in bwd}
        for _ in range(args.rounds):
            for k, f in bwd.items():
                tb[k].append(bench.time_kernel_events(f, args.iters, warmup=2, min_warm_ms=10) * 1e6)
        print(f"B={B} N={N} d={d} C={C} forward: " + "; ".join(_fmt(k, t) for k, t in tf.items())
              + f"; weighted / windowed {statistics.median(tf['weighted']) / statistics.median(tf['windowed']):.3f}x, weighted / matrix "
              f"{statistics.median(tf['weighted']) / statistics.median(tf['matrix']):.2f}x; peak extra memory "
              + ", ".join(f"{k} {v / 1e6:.2f} MB" for k, v in mem.items())
              + f"; largest |difference| of the weighted log-probabilities, fused vs matrix, {diff:.2e}", flush=True)
        print(f"B={B} N={N} d={d} C={C} forward + backward: " + "; ".join(_fmt(k, t) for k, t in tb.items())
              + f"; weighted / windowed {statistics.median(tb['weighted']) / statistics.median(tb['windowed']):.3f}x", flush=True)
        del q, s, bank, a
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
