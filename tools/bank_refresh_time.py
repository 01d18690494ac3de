"""Bringing R rows of a resident bank up to date: ops.SplitBank.update_rows (nw_bank_update_rows_f32: one launch, R rows
read and written) against the route without it -- the rows written by torch (full_feat.index_copy_, or the torch blend
with the old rows), then a new ops.SplitBank(full_feat, labels): all N rows read and written again, the labels checked with
a host synchronisation, the run tables rebuilt.

    python tools/bank_refresh_time.py [--iters 10] [--warmup 3] [--rounds 5] [--shapes 256x50000x512,256x400000x256] [--classes 200]

The two routes alternate in one process (the box is shared: a difference is only meaningful against the spread of the same
route, printed as min / median / max over the rounds); every round is timed with events on the stream around `iters` calls
(the rebuild's host synchronisation falls inside its interval, as it does in a training step).  Momentum 0 and 0.5 per
shape.  The bytes each route allocates (torch.cuda.max_memory_allocated over one call, above what was allocated before it)
are reported beside the times, and the two routes' banks are compared bit for bit.  One JSON line per shape and momentum.
Needs the MI355X: fails without one."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nwhead_amd import ops  # noqa: E402


def timed(step, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        step()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters      # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default="256x50000x512,256x400000x256")
    ap.add_argument("--classes", type=int, default=200)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bank_refresh_time measures on the MI355X"
    dev = torch.device("cuda:0")
    C = args.classes
    for shape in args.shapes.split(","):
        R, N, d = (int(v) for v in shape.split("x"))
        for momentum in (0.0, 0.5):
            g = torch.Generator().manual_seed(0)
            base = torch.randn(N, d, generator=g)
            sy = (torch.arange(N) % C).sort().values.to(dev)
            rows = torch.randperm(N, generator=g)[:R].to(dev)
            x = torch.randn(R, d, generator=g).to(dev)
            m = torch.tensor(momentum, dtype=torch.float32, device=dev)
            s_a, s_b = base.to(dev), base.to(dev)
            state = {"a": ops.SplitBank(s_a, labels=sy), "b": ops.SplitBank(s_b, labels=sy)}

            def update_rows():
                state["a"].update_rows(s_a, rows, x, momentum)

            def rebuild():
                if momentum == 0:
                    s_b.index_copy_(0, rows, x)
                else:
                    s_b.index_copy_(0, rows, m * s_b[rows] + (1 - m) * x)
                state["b"] = ops.SplitBank(s_b, labels=sy)

            routes = {"update_rows": update_rows, "index_copy_and_rebuild": rebuild}
            alloc = {}
            for name, step in routes.items():
                step()                                      # (first-call costs, and both banks one update ahead alike)
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats(dev)
                before = torch.cuda.memory_allocated(dev)
                step()
                torch.cuda.synchronize()
                alloc[name] = torch.cuda.max_memory_allocated(dev) - before
            same = all(torch.equal(getattr(state["a"], k).view(torch.int32), getattr(state["b"], k).view(torch.int32))
                       for k in ("split", "scale", "norm2")) and torch.equal(s_a.view(torch.int32), s_b.view(torch.int32))
            for step in routes.values():
                for _ in range(args.warmup):
                    step()
            torch.cuda.synchronize()
            times = {name: [] for name in routes}
            for _ in range(args.rounds):                    # alternate the routes
                for name, step in routes.items():
                    times[name].append(timed(step, args.iters))
            rec = {"shape": [R, N, d], "momentum": momentum, "iters": args.iters, "rounds": args.rounds, "banks_bit_identical": bool(same)}
            for name in routes:
                ts = times[name]
                rec[name] = {"us_min": round(min(ts), 1), "us_median": round(statistics.median(ts), 1), "us_max": round(max(ts), 1),
                             "allocated_bytes": int(alloc[name])}
            print(json.dumps(rec), flush=True)
            del state, s_a, s_b


if __name__ == "__main__":
    main()
