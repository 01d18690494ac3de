"""Neighbour search over a sharded bank, timed on one device: 256 queries x 50000 rows x 512, k = 10, the bank cut into
1 / 2 / 8 emulated shards (ShardedBanks of world 1 with explicit row_lo).  Per shard count (HIP events, median of the rounds
and their spread):
  * the per-shard search: ShardedBank.knn_partial, summed over the shards (one rank runs ONE of them);
  * the cross-shard step: ops.nw_knn_merge over the stacked candidates, with the head (C = 200);
  * for comparison the same step composed of torch.topk over the concatenated candidates + a gather of their labels +
    ops.nw_aggregate (no tie rule between equal scores).
Every shard count runs in a child process of its own under a time limit; the first one that fails ends the run.
  python tools/knn_sharded_time.py [--rounds R] [--iters I] [--limit SECONDS]"""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, N, D, K, C = 256, 50000, 512, 10, 200
SHARDS = (1, 2, 8)


def step(G, rounds, iters):
    import torch
    sys.path.insert(0, ROOT)
    import bench
    from nwhead_amd import ops
    from nwhead_amd.sharded import ShardedBank, shard_bounds

    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(N + K)
    q = torch.randn(B, D, generator=g).to(dev)
    s = torch.randn(N, D, generator=g).to(dev)
    sy = (torch.arange(N) % C).sort().values.to(dev)
    banks = []
    for r in range(G):
        lo, hi = shard_bounds(N, G, r)
        banks.append(ShardedBank(s[lo:hi], sy[lo:hi], C, row_lo=lo))
    st = torch.stack([b.knn_partial(q, K).view(3, B, K) for b in banks])          # (G, 3, B, K), as gathered
    vals, rows, labels = st[:, 0].view(torch.float32), st[:, 1], st[:, 2]

    def search():
        for b in banks:
            b.knn_partial(q, K)

    def merge():
        return ops.nw_knn_merge(vals, rows, labels, K, C)

    cat_v = vals.permute(1, 0, 2).reshape(B, G * K).contiguous()
    cat_r = rows.permute(1, 0, 2).reshape(B, G * K).contiguous()
    cat_y = labels.permute(1, 0, 2).reshape(B, G * K).to(torch.int64).contiguous()

    def composed():
        v, j = torch.topk(cat_v, K, dim=1)
        return torch.gather(cat_r, 1, j), ops.nw_aggregate(v, torch.gather(cat_y, 1, j), C)

    idx, _, _, out = merge()
    ridx, rout = composed()
    same_rows = bool((idx.sort(dim=1).values == ridx.to(torch.int64).sort(dim=1).values).all())
    err = float((out - rout).abs().max())
    res = {}
    for name, fn in (("search", search), ("merge", merge), ("torch.topk + nw_aggregate", composed)):
        ts = [bench.time_kernel_events(fn, iters, warmup=3, min_warm_ms=10) * 1e6 for _ in range(rounds)]
        res[name] = (statistics.median(ts), min(ts), max(ts))
    print(f"G={G}: " + "; ".join(f"{n} {m:.1f} us [{a:.1f}, {b:.1f}]" for n, (m, a, b) in res.items())
          + f"; search per shard {res['search'][0] / G:.1f} us; same rows as the composition: {same_rows}, "
          f"max |log-prob difference| {err:.2e}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--limit", type=int, default=180, help="seconds per shard count")
    ap.add_argument("--step", type=int, default=0, help="(internal) run one shard count in this process")
    args = ap.parse_args()
    if args.step:
        return step(args.step, args.rounds, args.iters)
    print(f"B={B} N={N} d={D} k={K} C={C}", flush=True)
    for G in SHARDS:
        r = subprocess.run(["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--step", str(G),
                            "--rounds", str(args.rounds), "--iters", str(args.iters)])
        if r.returncode != 0:
            sys.exit(f"G={G}: exit status {r.returncode}; nothing further is run")


if __name__ == "__main__":
    main()
