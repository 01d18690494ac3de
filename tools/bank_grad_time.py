"""Forward + backward of the head over a resident bank: ops.nw_head_bank (nw_bwd_query_f32, no (B,N) matrix, no support
gradient) against the route through the score matrix, ops.nw_head(q.requires_grad_(), s, sy, support_cache=bank).

    python tools/bank_grad_time.py [--iters 30] [--warmup 5] [--shapes 256x50000x512,256x400000x256] [--classes 200]

The two routes alternate in one process (the box is shared: a difference is only meaningful against the spread of the same
route, printed as min / median / max over the rounds); every round is timed with events on the stream around `iters`
forward + backward steps under the nll_loss gradient.  The leave-one-out variant of nw_head_bank (every query a bank row,
its own row excluded) is timed beside them -- the other route has no such mode.  Peak memory
(torch.cuda.max_memory_allocated, counter reset after the bank is built and the forward's scratch is warm) is reported per
route, and the two gradients are compared.  One JSON line per shape.  Needs the MI355X: fails without one."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nwhead_amd import ops  # noqa: E402


def timed(step, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        step()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters      # us per forward + backward


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default="256x50000x512,256x400000x256")
    ap.add_argument("--classes", type=int, default=200)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bank_grad_time measures on the MI355X"
    dev = torch.device("cuda:0")
    C = args.classes
    for shape in args.shapes.split(","):
        B, N, d = (int(v) for v in shape.split("x"))
        g = torch.Generator().manual_seed(0)
        s = torch.randn(N, d, generator=g).to(dev)
        sy = (torch.arange(N) % C).sort().values.to(dev)
        q0 = torch.randn(B, d, generator=g).to(dev)
        t = torch.randint(0, C, (B,), generator=g).to(dev)
        rows = torch.randperm(N, generator=g)[:B].to(dev)
        bank = ops.SplitBank(s, labels=sy)
        qloo = s[rows].clone()
        win = (rows, rows + 1)

        def make(fn, qsrc):
            q = qsrc.clone().requires_grad_(True)

            def step():
                q.grad = None
                F.nll_loss(fn(q), t).backward()
            return step, q

        routes = {
            "nw_head_bank": make(lambda q: ops.nw_head_bank(q, s, sy, C, bank), q0),
            "nw_head": make(lambda q: ops.nw_head(q, s, sy, C, support_cache=bank), q0),
            "nw_head_bank_loo": make(lambda q: ops.nw_head_bank(q, s, sy, C, bank, row_window=win, exclude=True), qloo),
        }
        peak = {}
        for name, (step, _) in routes.items():
            ops._WS_CACHE.clear()
            with torch.no_grad():                       # the forward's scratch, as every inference call leaves it
                ops.nw_head(q0, s, sy, C, support_cache=bank)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(dev)
            before = torch.cuda.memory_allocated(dev)
            step()
            torch.cuda.synchronize()
            peak[name] = torch.cuda.max_memory_allocated(dev) - before
        for step, _ in routes.values():
            for _ in range(args.warmup):
                step()
        torch.cuda.synchronize()
        times = {name: [] for name in routes}
        for _ in range(args.rounds):                    # alternate the routes
            for name, (step, _) in routes.items():
                times[name].append(timed(step, args.iters))
        ga, gb = routes["nw_head_bank"][1].grad, routes["nw_head"][1].grad
        rec = {"shape": [B, N, d, C], "iters": args.iters, "rounds": args.rounds, "score_matrix_bytes": 4 * B * N,
               "gq_max_abs_diff_over_max": float((ga - gb).abs().max() / gb.abs().max())}
        for name in routes:
            ts = times[name]
            rec[name] = {"us_min": round(min(ts), 1), "us_median": round(statistics.median(ts), 1), "us_max": round(max(ts), 1),
                         "peak_bytes": int(peak[name])}
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
