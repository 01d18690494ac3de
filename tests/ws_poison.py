"""Poisoned scratch buffers for the tests of the fused forward (a plain helper module, imported by the GPU tests).

The tile kernels write per-tile partials (FusedWs in nwhead_amd/csrc/fused_impl.h: m, den, num) into a scratch buffer that
nw_merge_runs_kernel then reads.  The product never clears that buffer: ops._workspace() keeps one tensor per (device,
stream) and only grows it, ShardedBank keeps its own `_ws`, and the layout depends on the shape alone -- so a store that a
kernel forgets is filled in, bit for bit, by the previous call of the same shape.  A test that compares two calls, or one
call with a reference after an earlier call of the same shape, must therefore poison the buffer first.

The poison is byte 0xFF: NaN as a float, -1 as an int.  The merge takes the tile maxima with fmaxf, which drops a NaN, so a
missing tile shows through `den` and `num`, not through `m`: callers assert torch.isfinite(out).all() next to their
comparison.  (Run tables are rewritten by every launch or live in the bank, the split queries are rewritten by every
launch, and rows of `num` at or past a tile's run count are never read: correct kernels give finite outputs.)
"""
import torch


def poison_cached_workspaces(min_bytes=0, device=None):
    """Fill every tensor of ops._WS_CACHE with 0xFF; returns the number of bytes filled (assert it: 0 means a no-op).

    min_bytes / device: first make the cached buffer of `device`'s current stream hold at least `min_bytes`, through
    the product's own accessor -- a call that needs more than the cache holds would otherwise allocate a fresh,
    unpoisoned tensor (typically the block the allocator has just taken back, stale partials included)."""
    from nwhead_amd import ops
    if min_bytes and device is not None:
        ops._workspace(int(min_bytes), device)
    filled = 0
    for ws in ops._WS_CACHE.values():
        ws.fill_(0xFF)
        filled += ws.numel() * ws.element_size()
    return filled


def poisoned_workspace(nbytes, dev):
    """A fresh 0xFF-filled uint8 tensor: `ws=` of ops.nw_partials_into, or ShardedBank._ws."""
    return torch.full((max(int(nbytes), 1),), 0xFF, dtype=torch.uint8, device=dev)


def fwd_workspace_bytes(B, N, d, C):
    """What the forward asks for at this shape (nw_fwd_workspace_bytes)."""
    from nwhead_amd import _lib
    return int(_lib.load().nw_fwd_workspace_bytes(int(B), int(N), int(d), int(C)))
