"""A training step of the class head with LEARNABLE BANK ROWS (forward + backward under nll_loss, C = 200) over a resident
bank, routes alternated in one process:
  * fused:   ops.nw_head_bank(q, s, sy, C, bank, support_grad=True) -> the inference call forward, nw_bwd_bank_support_f32
             backward; no (B,N) matrix;
  * matrix:  ops.nw_head(q, s.requires_grad_(), sy, C, support_cache=bank), the route the rows had before the keyword, which
             saves a (B,N) score matrix and fills two more in its workspace.
Only the rows learn in both.  Per shape: us per step (HIP events, median of the rounds and their spread), the peak extra
device memory of one step of each route (every workspace warmed first), and how the two gradients compare.
  python tools/bank_support_grad_time.py [--rounds R] [--iters I]         (NW_SPLIT_ALWAYS unset)"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from nwhead_amd import ops

SHAPES = ((256, 50000, 512), (256, 400000, 256), (4096, 2048, 512))      # the last one: a prototype set
C = 200


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
    for B, N, d in SHAPES:
        g = torch.Generator().manual_seed(N + d)
        s = torch.randn(N, d, generator=g).to(dev).requires_grad_(True)
        sy = (torch.arange(N) % C).sort().values.to(dev)
        bank = ops.SplitBank(s, labels=sy)
        q = torch.randn(B, d, generator=g).to(dev)
        t = torch.randint(0, C, (B,), generator=g).to(dev)
        assert ops.head_bank_support_route(split=bank.split is not None, sorted_copy=bank.sorted_rows is not None,
                                           shape=bank.shape, pad=bank.pad, width=d, B=B, n_classes=C) == "fused"

        def fused():
            s.grad = None
            F.nll_loss(ops.nw_head_bank(q, s, sy, C, bank, support_grad=True), t).backward()
            return s.grad

        def matrix():
            s.grad = None
            F.nll_loss(ops.nw_head(q, s, sy, C, support_cache=bank), t).backward()
            return s.grad

        routes = {"fused": fused, "matrix": matrix}
        for f in routes.values():          # (every route once: its workspaces are cached before memory is looked at)
            f()
        gf = fused().clone()
        gm = matrix()
        diff = float((gf - gm).abs().max() / gm.abs().max())
        del gf, gm
        mem = {k: _peak_extra(f) for k, f in routes.items()}
        tm = {k: [] for k in routes}
        for _ in range(args.rounds):
            for k, f in routes.items():
                tm[k].append(bench.time_kernel_events(f, args.iters, warmup=2, min_warm_ms=10) * 1e6)
        med = {k: statistics.median(x) for k, x in tm.items()}
        print(f"B={B} N={N} d={d} C={C}: " + "; ".join(_fmt(k, x) for k, x in tm.items())
              + f"; fused / matrix {med['fused'] / med['matrix']:.2f}x"
              + "; peak extra memory " + ", ".join(f"{k} {x / 1e6:.2f} MB" for k, x in mem.items())
              + f" (gs itself: {N * d * 4 / 1e6:.2f} MB, one score matrix: {B * N * 4 / 1e6:.2f} MB)"
              + f"; largest |gs fused - gs matrix| / max|gs matrix| {diff:.2e}", flush=True)
        s.grad = None
        del s, bank, q, routes
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
