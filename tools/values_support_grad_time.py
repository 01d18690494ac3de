"""A training step of the value head with LEARNABLE values and support weights (forward + backward) over a resident bank,
routes alternated in one process:
  * fused:        ops.nw_head_values_bank(support_grad=True) -> the lse pass and nw_fwd_values_f32 forward,
                  nw_bwd_values_support_f32 (and nw_bwd_values_query_f32 when the queries learn) backward; no (B,N) matrix;
  * composition:  the hand-written ops.nw_scores over the bank, + row_logw, torch.softmax and a matmul with the values under
                  torch autograd -- what a caller has to write without the keyword -- which keeps three (B,N) matrices.
Three steps of each: (a) the values learn, (b) the weights alone learn, (c) values, weights and queries learn.
Per shape and per T in {32, 512}: us per step (HIP events, median of the rounds and their spread), the peak extra device
memory of one step of each route, and how the gradients of the two routes compare.
  python tools/values_support_grad_time.py [--rounds R] [--iters I]         (NW_SPLIT_ALWAYS unset)"""
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
        bank = ops.SplitBank(s, labels=(torch.arange(N) % 10).sort().values.to(dev))
        q0 = torch.randn(B, d, generator=g).to(dev)
        a0 = (0.5 * torch.randn(N, generator=g)).to(dev)
        for T in WIDTHS:
            v0 = torch.randn(N, T, generator=g).to(dev)
            gout = torch.randn(B, T, generator=g).to(dev)
            assert ops.head_values_grad_route(split=bank.split is not None, sorted_copy=bank.sorted_rows is not None,
                                              shape=bank.shape, pad=bank.pad, width=d, B=B, T=T) == "fused"
            # the leaves of the three steps: (values, weights, queries) learn
            modes = {"values": (True, False, False), "weights": (False, True, False), "all": (True, True, True)}
            routes, leaves = {}, {}
            for mode, (lv, la, lq) in modes.items():
                v, a, q = v0.clone().requires_grad_(lv), a0.clone().requires_grad_(la), q0.clone().requires_grad_(lq)
                vals = ops.BankValues(v, bank)           # prepared once: a loop that steps the values refreshes it in place
                leaves[mode] = [t for t in (v, a, q) if t.requires_grad]

                def fused(vals=vals, a=a, q=q, mode=mode):
                    for t in leaves[mode]:
                        t.grad = None
                    ops.nw_head_values_bank(q, s, bank, vals, row_logw=a, support_grad=True).backward(gout)
                    return [t.grad for t in leaves[mode]]

                def composition(v=v, a=a, q=q, mode=mode):
                    for t in leaves[mode]:
                        t.grad = None
                    ops._values_head_matrix(q, s, bank, v, "euclidean", None, a, None, None, False).backward(gout)
                    return [t.grad for t in leaves[mode]]

                routes[f"fused {mode}"], routes[f"composition {mode}"] = fused, composition
            for f in routes.values():          # (every route once: its workspaces are cached before memory is looked at)
                f()
            diff = {}
            for mode in modes:
                gf = [x.clone() for x in routes[f"fused {mode}"]()]
                gm = routes[f"composition {mode}"]()
                diff[mode] = max(float((x - y).abs().max() / y.abs().max()) for x, y in zip(gf, gm))
                del gf, gm
            mem = {k: _peak_extra(f) for k, f in routes.items()}
            t = {k: [] for k in routes}
            for _ in range(args.rounds):
                for k, f in routes.items():
                    t[k].append(bench.time_kernel_events(f, args.iters, warmup=2, min_warm_ms=10) * 1e6)
            med = {k: statistics.median(x) for k, x in t.items()}
            print(f"B={B} N={N} d={d} T={T}: " + "; ".join(_fmt(k, x) for k, x in t.items()) + "; fused / composition "
                  + ", ".join(f"{m} {med['fused ' + m] / med['composition ' + m]:.2f}x" for m in modes)
                  + "; peak extra memory " + ", ".join(f"{k} {x / 1e6:.2f} MB" for k, x in mem.items())
                  + "; largest |g fused - g composition| / max|g composition| "
                  + ", ".join(f"{m} {x:.2e}" for m, x in diff.items()), flush=True)
            for mode in modes:
                for x in leaves[mode]:
                    x.grad = None
            del routes, leaves, v0, gout
            torch.cuda.empty_cache()
        del s, bank, q0, a0
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
