"""The half-precision bank against the fp32-grade (split-fp16) bank on the K3 shape: nw_head over a resident bank of
50000 x 512 with 200 classes, B = 6656 and B = 256 queries.

Both banks live in ONE process and their timed windows ALTERNATE (fp32, fp16, fp32, fp16, ...), so clock state, other
tenants of the host and allocator state hit both alike; every window is device time between two HIP events around
back-to-back calls (at least ~50 ms of work), taken after a warm-up of both paths.  Reported per shape: the median and
the min-max spread of the windows of each bank, the ratio of the medians, and max |log-prob difference| between the two
heads on the same inputs (the fp16 head is the head of the fp16-rounded features, not an approximation of the kernel).

    python tools/half_bank_bench.py [--rounds 7] [--json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nwhead_amd import _lib, ops  # noqa: E402

N, D, C = 50000, 512, 200


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3      # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--json", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    _lib.check(_lib.load().nw_device_check(), "nw_device_check")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    s = torch.randn(N, D, generator=g).to(dev)
    sy = (torch.arange(N) * C // N).to(dev)          # class-sorted, 250 rows per class
    banks = {"fp32": ops.SplitBank(s, labels=sy), "fp16": ops.SplitBank(s, labels=sy, precision="fp16")}
    results = []
    for B in (6656, 256):
        q = (torch.randn(B, D, generator=g) * 0.7).to(dev)
        fns = {k: (lambda b=b: ops.nw_head(q, s, sy, C, support_cache=b)) for k, b in banks.items()}
        outs = {k: fn().clone() for k, fn in fns.items()}
        torch.cuda.synchronize()
        iters = {}
        for k, fn in fns.items():                    # warm-up, and the window length that gives ~50 ms
            window(fn, 5)
            iters[k] = max(10, int(50e3 / window(fn, 10)))
        times = {k: [] for k in fns}
        for _ in range(args.rounds):
            for k, fn in fns.items():
                times[k].append(window(fn, iters[k]))
        med = {k: statistics.median(v) for k, v in times.items()}
        r = {"B": B, "N": N, "d": D, "C": C, "rounds": args.rounds,
             "fp32_us": med["fp32"], "fp32_min_us": min(times["fp32"]), "fp32_max_us": max(times["fp32"]),
             "fp16_us": med["fp16"], "fp16_min_us": min(times["fp16"]), "fp16_max_us": max(times["fp16"]),
             "speedup": med["fp32"] / med["fp16"],
             "max_abs_dlogp": (outs["fp16"] - outs["fp32"]).abs().max().item(),
             "bank_bytes_fp32": banks["fp32"].split.numel() * 4, "bank_bytes_fp16": banks["fp16"].packed.numel() * 2}
        results.append(r)
        if not args.json:
            print(f"B={B:5d}: fp32-grade {r['fp32_us']:8.1f} us [{r['fp32_min_us']:.1f}, {r['fp32_max_us']:.1f}]   "
                  f"fp16 {r['fp16_us']:8.1f} us [{r['fp16_min_us']:.1f}, {r['fp16_max_us']:.1f}]   "
                  f"x{r['speedup']:.3f}   max |dlogp| {r['max_abs_dlogp']:.3e}")
    if args.json:
        print(json.dumps(results))


if __name__ == "__main__":
    main()
