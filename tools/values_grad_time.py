"""A training step of the value head (forward + backward w.r.t. the queries) over a resident bank, routes alternated in one
process:
  * fused:   ops.nw_head_values_bank with a prepared ops.BankValues -> the lse pass and nw_fwd_values_f32 forward,
             nw_bwd_values_query_f32 backward; no (B,N) matrix;
  * matrix:  the autograd composition ops.nw_scores over the bank, torch.softmax and a matmul with the values (what
             nw_head_values_bank falls back to), which keeps three (B,N) matrices;
  * floor:   forward + backward of ops.nw_head_bank (10 classes) over the same bank -- the same skeleton without the
             G V^T product; bwd_values_plan's cost model puts the value head's backward 3 T/32 per support tile above it.
Per shape and per T in {32, 512}: us per step (HIP events, median of the rounds and their spread), the forward alone of the
fused route and of the floor (step - forward = the backward), the peak extra device memory of one step of each route, and
how the two gradients compare.
  python tools/values_grad_time.py [--rounds R] [--iters I]         (NW_SPLIT_ALWAYS unset)"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from nwhead_amd import ops

SHAPES = ((256, 50000, 512), (256, 400000, 256))
WIDTHS = (32, 512)
CLASSES = 10


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
        s = torch.randn(N, d, generator=g).to(dev)
        sy = (torch.arange(N) % CLASSES).sort().values.to(dev)
        bank = ops.SplitBank(s, labels=sy)
        q = torch.randn(B, d, generator=g).to(dev).requires_grad_(True)
        gc = torch.randn(B, CLASSES, generator=g).to(dev)

        def step(forward, gout):
            def run():
                q.grad = None
                forward().backward(gout)
                return q.grad
            return run

        def floor_fwd():
            return ops.nw_head_bank(q, s, sy, CLASSES, bank)

        for T in WIDTHS:
            v = torch.randn(N, T, generator=g).to(dev)
            gout = torch.randn(B, T, generator=g).to(dev)
            vals = ops.BankValues(v, bank)
            assert ops.head_values_grad_route(split=bank.split is not None, sorted_copy=bank.sorted_rows is not None,
                                              shape=bank.shape, pad=bank.pad, width=d, B=B, T=T) == "fused"

            def fused_fwd():
                return ops.nw_head_values_bank(q, s, bank, vals)

            def matrix_fwd():
                return ops._values_head_matrix(q, s, bank, v, "euclidean", None, None, None, None, False)

            def inference(forward):
                def run():
                    with torch.no_grad():
                        return forward()
                return run

            routes = {"fused": step(fused_fwd, gout), "matrix": step(matrix_fwd, gout), "floor": step(floor_fwd, gc),
                      "fused forward": inference(fused_fwd), "floor forward": inference(floor_fwd)}
            for f in routes.values():          # (every route once: its workspaces are cached before memory is looked at)
                f()
            gf, gm = routes["fused"]().clone(), routes["matrix"]().clone()
            diff = float((gf - gm).abs().max() / gm.abs().max())
            del gf, gm
            mem = {k: _peak_extra(routes[k]) for k in ("fused", "matrix", "floor")}
            t = {k: [] for k in routes}
            for _ in range(args.rounds):
                for k, f in routes.items():
                    t[k].append(bench.time_kernel_events(f, args.iters, warmup=2, min_warm_ms=10) * 1e6)
            med = {k: statistics.median(x) for k, x in t.items()}
            print(f"B={B} N={N} d={d} T={T}: " + "; ".join(_fmt(k, x) for k, x in t.items())
                  + f"; fused / matrix {med['fused'] / med['matrix']:.2f}x; backward alone: fused {med['fused'] - med['fused forward']:.1f} us,"
                  f" floor {med['floor'] - med['floor forward']:.1f} us; peak extra memory "
                  + ", ".join(f"{k} {x / 1e6:.2f} MB" for k, x in mem.items())
                  + f"; largest |gq fused - gq matrix| / max|gq matrix| {diff:.2e}", flush=True)
            del v, vals, gout
            q.grad = None
            torch.cuda.empty_cache()
        del q, s, bank
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
