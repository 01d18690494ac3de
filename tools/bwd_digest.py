"""SHA-256 of the head's gradients (gq, gs, glogit_scale) at fixed seeds, for comparing two builds of the library bit for bit
(NW_HIP_LIB names another build): the backward is deterministic, so a refactor of its host code must leave every line as
it was.  python tools/bwd_digest.py [group ...]

Without arguments every group runs in a process of its own under its own time limit, and the first failure ends the run.
Groups: the three SHAPES of tests/test_head_backward_gpu.py and its three poison shapes, each on the three product routes
and with all five score kinds; the benchmark's T shape on the default route; per-query supports."""
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("euclidean", "hypersphere_euclidean", "cosine", "dotproduct", "clip")
ROUTE_ENV = {"valu": {"NW_BWD_NO_MFMA": "1"}, "mfma": {"NW_BWD_SPLIT": "0"}, "split": {"NW_BWD_SPLIT": "1"}, "default": {}}
THREE = ("valu", "mfma", "split")
GROUPS = {   # name -> (shape, per-query supports, routes, kinds, seconds allowed)
    "s64x1024x64": ((64, 1024, 64, 5), False, THREE, KINDS, 120),
    "s129x257x160": ((129, 257, 160, 1000), False, THREE, KINDS, 120),
    "s33x4099x64": ((33, 4099, 64, 7), False, THREE, KINDS, 120),
    "p64x1024x96": ((64, 1024, 96, 5), False, THREE, KINDS, 120),
    "p256x512x64": ((256, 512, 64, 5), False, THREE, KINDS, 120),
    "T": ((256, 10000, 512, 200), False, ("default",), KINDS, 120),
    "perquery": ((3, 3000, 36, 7), True, ("default",), KINDS, 120),
}   # (the first poison shape is the first of SHAPES)


def digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()[:16]


def run_group(name):
    import torch
    sys.path.insert(0, ROOT)
    from nwhead_amd import _lib, ops
    (B, N, d, C), batched, routes, kinds, _ = GROUPS[name]
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(B + N + d)
    q0 = torch.randn(B, d, generator=g)
    s0 = torch.randn(B, N, d, generator=g) if batched else torch.randn(N, d, generator=g)
    sy = torch.randint(0, C, (B, N) if batched else (N,), generator=g).to(dev)
    G = torch.randn(B, C, generator=g).to(dev)
    for kind in kinds:
        k = d ** -0.25 if kind == "dotproduct" else 1.0
        for route in routes:
            for v in ("NW_BWD_NO_MFMA", "NW_BWD_SPLIT"):
                os.environ.pop(v, None)
            os.environ.update(ROUTE_ENV[route])
            _lib.sync_knobs()
            q, s = (q0 * k).to(dev).requires_grad_(True), (s0 * k).to(dev).requires_grad_(True)
            ls = torch.tensor(2.659260036932778, device=dev, requires_grad=True) if kind == "clip" else None
            (ops.nw_head(q, s, sy, C, kind, ls) * G).sum().backward()
            torch.cuda.synchronize()
            gls = digest(ls.grad) if ls is not None else "-"
            print(f"DIGEST {name:13s} {route:7s} {kind:21s} gq {digest(q.grad)} gs {digest(s.grad)} gls {gls}", flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1:
        for name in sys.argv[1:]:
            run_group(name)
        sys.exit(0)
    for name, spec in GROUPS.items():
        r = subprocess.run([sys.executable, os.path.abspath(__file__), name], timeout=spec[-1])
        if r.returncode != 0:
            sys.exit(f"bwd_digest: group {name} ended with status {r.returncode}: nothing more is started")
