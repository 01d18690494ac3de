"""A training step of the VALUE head with LEARNABLE BANK ROWS (forward + backward under mse_loss) over a resident bank,
routes alternated in one process:
  * fused:   ops.nw_head_values_bank(q, s, bank, values, support_grad=True) -> the inference launches forward,
             nw_bwd_values_bank_support_f32 (and nw_bwd_values_query_f32 / nw_bwd_values_support_f32 when the queries and the
             values learn too) backward; no (B,N) matrix;
  * matrix:  the "matrix" composition ops._values_head_matrix with `s` a leaf -- nw_scores through ops._ScoresFn, + the mask,
             torch.softmax and a matmul under torch autograd, which keeps (B,N) matrices;
  * torch:   (--torch) the same composition in plain torch ops: -torch.cdist, softmax, matmul.
Two modes per shape: only the rows learn ("rows"); the rows, the values and the queries learn ("all").  Per shape and mode: us
per step (HIP events, median of the rounds and their spread), the peak extra device memory of one step of each route (every
workspace warmed first), and how the gradients to the rows compare.
  python tools/values_bank_grad_time.py [--rounds R] [--iters I] [--torch]         (NW_SPLIT_ALWAYS unset)"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from nwhead_amd import ops

# (B, N, d, T); the last one: a prototype set
SHAPES = ((256, 50000, 512, 32), (256, 50000, 512, 512), (256, 400000, 256, 32), (256, 400000, 256, 512), (4096, 2048, 512, 32))


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
    ap.add_argument("--torch", action="store_true", help="time the pure-torch composition beside the two")
    ap.add_argument("--shapes", type=int, nargs="*", help="indices into SHAPES (default: all)")
    args = ap.parse_args()
    if os.environ.get("NW_SPLIT_ALWAYS"):
        raise SystemExit("run with NW_SPLIT_ALWAYS unset")
    dev = torch.device("cuda:0")
    for B, N, d, T in (SHAPES if not args.shapes else [SHAPES[i] for i in args.shapes]):
        g = torch.Generator().manual_seed(N + d + T)
        s = torch.randn(N, d, generator=g).to(dev).requires_grad_(True)
        bank = ops.SplitBank(s)
        v = torch.randn(N, T, generator=g).to(dev)
        q = torch.randn(B, d, generator=g).to(dev)
        t = torch.randn(B, T, generator=g).to(dev)
        assert ops.head_values_grad_route(split=bank.split is not None, sorted_copy=bank.sorted_rows is not None,
                                          shape=bank.shape, pad=bank.pad, width=d, B=B, T=T) == "fused"
        for mode in ("rows", "all"):
            learn = mode == "all"
            q.requires_grad_(learn)
            v.requires_grad_(learn)
            vals = ops.BankValues(v, bank)

            def step(out_fn):
                s.grad = q.grad = v.grad = None
                F.mse_loss(out_fn(), t).backward()
                return s.grad

            def fused():
                return step(lambda: ops.nw_head_values_bank(q, s, bank, vals, support_grad=True))

            def matrix():
                return step(lambda: ops._values_head_matrix(q, s, bank, v, "euclidean", None, None, None, None, False))

            def plain():
                return step(lambda: torch.softmax(-torch.cdist(q, s), dim=1) @ v)

            routes = {"fused": fused, "matrix": matrix}
            if args.torch:
                routes["torch"] = plain
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
            print(f"B={B} N={N} d={d} T={T} {mode}: " + "; ".join(_fmt(k, x) for k, x in tm.items())
                  + f"; fused / matrix {med['fused'] / med['matrix']:.2f}x"
                  + "; peak extra memory " + ", ".join(f"{k} {x / 1e6:.2f} MB" for k, x in mem.items())
                  + f" (gs itself: {N * d * 4 / 1e6:.2f} MB, one score matrix: {B * N * 4 / 1e6:.2f} MB)"
                  + f"; largest |gs fused - gs matrix| / max|gs matrix| {diff:.2e}", flush=True)
            s.grad = q.grad = v.grad = None
            del vals, routes
        del s, bank, q, v
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
