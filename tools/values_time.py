"""The value head (Nadaraya-Watson regression: softmax(scores) @ values) over a resident bank, routes alternated in one process:
  * fused:      ops.nw_head_values with a prepared ops.BankValues -> the forward's lse pass (nw_fwd_window_f32 over all-zero
                labels, one class, the whole bank as the kept window) and nw_fwd_values_f32; no (B,N) matrix;
  * lse pass:   that first launch alone (ops.nw_head_window over the same labels and window);
  * value pass: nw_fwd_values_f32 alone, through ctypes, with the lse of the first pass -- what a single-pass (online softmax)
                variant would have to beat is fused - value pass;
  * matrix:     ops.nw_scores over the bank, torch.softmax and a matmul with the values: what the value head falls back to,
                with its (B,N) matrix held twice.
Per shape and per T in {32, 512}: us per call (HIP events, median of the rounds and their spread), the peak extra device
memory of one call of the fused and the matrix route, and how their answers compare.
  python tools/values_time.py [--rounds R] [--iters I]         (NW_SPLIT_ALWAYS unset)"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from nwhead_amd import _lib, ops

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
    lib = _lib.load()
    for B, N, d in SHAPES:
        g = torch.Generator().manual_seed(N + d)
        s = torch.randn(N, d, generator=g).to(dev)
        bank = ops.SplitBank(s)
        q = torch.randn(B, d, generator=g).to(dev)
        zeros = torch.zeros(N, dtype=torch.int64, device=dev)
        whole = (torch.zeros(B, dtype=torch.int32, device=dev), torch.full((B,), N, dtype=torch.int32, device=dev))
        for T in WIDTHS:
            v = torch.randn(N, T, generator=g).to(dev)
            vals = ops.BankValues(v, bank)
            assert ops.head_values_route(split=bank.split is not None, sorted_copy=bank.sorted_rows is not None, shape=bank.shape,
                                         pad=bank.pad, width=d, B=B, T=T) == "fused"
            with torch.no_grad():
                _, lse = ops.nw_head_values(q, s, bank, vals, return_lse=True)
                out = torch.empty(B, vals.width, device=dev)
                ws_bytes = lib.nw_fwd_values_workspace_bytes(B, N, d, vals.width, 0)
                ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
                st = torch.cuda.current_stream(dev).cuda_stream

                def value_pass():
                    _lib.check(lib.nw_fwd_values_f32(q.data_ptr(), bank.split.data_ptr(), bank.scale.data_ptr(), bank.norm2.data_ptr(),
                                                     vals.split.data_ptr(), vals.scale.data_ptr(), None, None, None, 0, lse.data_ptr(),
                                                     out.data_ptr(), ws.data_ptr(), ws_bytes, B, N, d, vals.width, 0, None, 0, st),
                               "nw_fwd_values_f32")
                    return out

                routes = {
                    "fused": lambda: ops.nw_head_values(q, s, bank, vals),
                    "lse pass": lambda: ops.nw_head_window(q, s, zeros, 1, bank, whole),
                    "value pass": value_pass,
                    "matrix": lambda: torch.softmax(ops.nw_scores(q, s, support_cache=bank), dim=1) @ v,
                }
                fused, matrix = routes["fused"](), routes["matrix"]()
                diff = float((fused - matrix).abs().max() / matrix.abs().max())
                del fused, matrix
                mem = {k: _peak_extra(routes[k]) for k in ("fused", "matrix")}
                t = {k: [] for k in routes}
                for _ in range(args.rounds):
                    for k, f in routes.items():
                        t[k].append(bench.time_kernel_events(f, args.iters, warmup=2, min_warm_ms=10) * 1e6)
            print(f"B={B} N={N} d={d} T={T}: " + "; ".join(_fmt(k, x) for k, x in t.items())
                  + f"; fused / matrix {statistics.median(t['fused']) / statistics.median(t['matrix']):.2f}x; workspace of the value pass "
                  f"{ws_bytes / 1e6:.2f} MB; peak extra memory " + ", ".join(f"{k} {x / 1e6:.2f} MB" for k, x in mem.items())
                  + f"; prepared values {2 * vals.rows.numel() * 4 / 1e6:.1f} MB; largest |fused - matrix| / max|matrix| {diff:.2e}", flush=True)
            del v, vals, out, ws
            torch.cuda.empty_cache()
        del q, s, bank
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
