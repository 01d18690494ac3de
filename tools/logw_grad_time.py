"""The gradient of the weighted head w.r.t. the support weights (ops.nw_head_bank(row_logw=a), a.requires_grad ->
nw_bwd_query_logw_f32), routes alternated in one process, forward + backward under nll_loss:
  (a) only the weights learn (a frozen featurizer):
      * fused:  nw_fwd_weighted_f32 + the weights-only kernel (no second pass over the bank rows, no (B,N) buffer);
      * matrix: ops.nw_aggregate(ops.nw_scores(q, s, support_cache=bank) + a, sy, C) with its backward -- the only way to
        this gradient before the kernel, through (B,N) matrices;
      with the time and the peak extra device memory (torch.cuda.max_memory_allocated) of one step of each;
  (b) queries and weights learn against the queries alone, in the same library:
      * gq + ga: nw_bwd_query_logw_f32 with gq;
      * gq:      nw_bwd_query_weighted_f32, the existing weighted backward.
Weights: finite, a_j by j mod 7 = {0, ln 2, -3.5, -1, 0, 1.25, -0.5} (learnable weights hold no -inf).
Per shape: us per step (HIP events, median of the rounds and their spread).
  python tools/logw_grad_time.py [--rounds R] [--iters I]         (NW_SPLIT_ALWAYS unset)"""
import argparse
import math
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from nwhead_amd import ops

SHAPES = ((256, 50000, 512, 200), (256, 400000, 256, 200))
PATTERN = (0.0, math.log(2.0), -3.5, -1.0, 0.0, 1.25, -0.5)


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
        t = torch.randint(0, C, (B,), generator=g).to(dev)
        facts = dict(split=bank.split is not None, sorted_copy=bank.sorted_rows is not None, shape=bank.shape, pad=bank.pad,
                     width=d, B=B, n_classes=C)
        assert ops.head_weighted_route(**facts, grad_logw=True) == "fused"

        def step(head, grad_q, grad_a):
            def run():
                qg = q.detach().requires_grad_(grad_q)
                ag = a.detach().requires_grad_(grad_a)
                F.nll_loss(head(qg, ag), t).backward()
                return qg.grad, ag.grad
            return run

        fused = lambda qg, ag: ops.nw_head_bank(qg, s, sy, C, bank, row_logw=ag)                      # noqa: E731
        matrix = lambda qg, ag: ops.nw_aggregate(ops.nw_scores(qg, s, support_cache=bank) + ag, sy, C)   # noqa: E731
        routes = {
            "(a) weights only, fused": step(fused, False, True),
            "(a) weights only, nw_scores + a + nw_aggregate": step(matrix, False, True),
            "(b) gq + ga": step(fused, True, True),
            "(b) gq alone": step(fused, True, False),
        }
        ga_f, ga_m = routes["(a) weights only, fused"]()[1], routes["(a) weights only, nw_scores + a + nw_aggregate"]()[1]
        diff = float((ga_f - ga_m).abs().max() / ga_m.abs().max())
        mem = {k: _peak_extra(f) for k, f in routes.items()}
        times = {k: [] for k in routes}
        for _ in range(args.rounds):
            for k, f in routes.items():
                times[k].append(bench.time_kernel_events(f, args.iters, warmup=2, min_warm_ms=10) * 1e6)
        med = {k: statistics.median(v) for k, v in times.items()}
        ka, km, kb, kq = routes
        print(f"B={B} N={N} d={d} C={C} forward + backward: " + "; ".join(_fmt(k, v) for k, v in times.items())
              + f"; (a) fused / matrix {med[ka] / med[km]:.2f}x; (b) (gq + ga) / gq {med[kb] / med[kq]:.3f}x; peak extra memory "
              + ", ".join(f"{k} {v / 1e6:.2f} MB" for k, v in mem.items())
              + f" (one score matrix {B * N * 4 / 1e6:.1f} MB); largest |difference| of ga, fused vs matrix, over max |ga| {diff:.2e}",
              flush=True)
        del q, s, bank, a
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
