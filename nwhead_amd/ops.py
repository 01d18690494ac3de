"""Tensor-level entry points over the C ABI: forward/backward of the NW head, scores, sharded
partials + merge, support influence.  PyTorch is plumbing only (device memory, current stream,
autograd bookkeeping); every arithmetic step runs in libnwhead_hip.so.
"""
from __future__ import annotations

import collections
import ctypes
import os
import weakref

import torch
from torch.autograd.function import once_differentiable

from . import _lib
from ._lib import SCORE_KINDS, NWHipError


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream(t: torch.Tensor):
    """The current HIP stream of t's device as the integer handle the C ABI takes (torch.cuda.current_stream builds
    a Python Stream object per call: ~4 us; the raw getter is what it wraps)."""
    if _raw_stream is not None:
        idx = t.device.index
        return _raw_stream(torch.cuda.current_device() if idx is None else idx)
    return torch.cuda.current_stream(t.device).cuda_stream


class _OnDevice:
    """`with torch.cuda.device(dev)` only when `dev` is not already the current device (the context manager costs
    several microseconds per call; the C ABI launches on the CURRENT device)."""
    __slots__ = ("ctx",)

    def __init__(self, dev):
        idx = dev.index
        self.ctx = None if (idx is None or idx == torch.cuda.current_device()) else torch.cuda.device(dev)

    def __enter__(self):
        if self.ctx is not None:
            self.ctx.__enter__()

    def __exit__(self, *a):
        if self.ctx is not None:
            self.ctx.__exit__(*a)


def _sig(t):
    """(storage address, shape, in-place version) of a tensor: what 'the very tensor, unmodified' means for the cached
    banks and run tables.  Inference tensors (torch.inference_mode) carry no version counter: None stands in."""
    return (t.data_ptr(), tuple(t.shape), _ver(t))


def _ver(t):
    """In-place version of a tensor, None for inference tensors (they have no counter and cannot be written in place
    outside inference mode; a replaced one shows up in its address)."""
    return None if t.is_inference() else t._version


_WS_BYTES = {}


def _fwd_ws_bytes(lib, B, N, d, C):
    key = (B, N, d, C)
    v = _WS_BYTES.get(key)
    if v is None:
        if len(_WS_BYTES) > 4096:
            _WS_BYTES.clear()
        v = _WS_BYTES[key] = lib.nw_fwd_workspace_bytes(B, N, d, C)
    return v


def _ptr(t):
    return None if t is None else t.data_ptr()


def _need_hip(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise NWHipError(
                "nwhead_amd ops run on MI355X only: got a CPU tensor. Move the module and its "
                "inputs to the HIP device (there is no CPU fallback in the product path).")


def _f32c(t):
    if t.dtype == torch.float32 and t.is_contiguous():
        return t.detach() if t.requires_grad else t
    return t.detach().to(torch.float32).contiguous()


def _i64c(t):
    """Labels (or rows) as the library reads them: int64, contiguous; the caller's own tensor when it already is."""
    return t if (t.dtype == torch.int64 and t.is_contiguous()) else t.detach().to(torch.int64).contiguous()


def _kind_id(kind):
    if isinstance(kind, int):
        return kind
    try:
        return SCORE_KINDS[kind]
    except KeyError:
        raise NotImplementedError(kind)


_WS_CACHE = {}
_OPTS = {}


def _default_opts(persistent_wgs=0, operand_form=0):
    """The nw_fwd_opts of a call without cached run tables (kept alive here; NW_SPLIT_ALWAYS read when first needed)."""
    key = (int(persistent_wgs), _lib.force_split(), int(operand_form))
    op = _OPTS.get(key)
    if op is None:
        op = _OPTS[key] = _lib.fwd_opts(persistent_wgs=persistent_wgs, operand_form=operand_form)
    return C_addr(op)


def C_addr(op):
    return ctypes.addressof(op)


def _workspace(nbytes, device, stream=None):
    """Scratch for one call.  Cached per (device, stream) and only ever grown: work on one stream is
    ordered, so the next call may reuse it; another stream gets its own."""
    nbytes = max(int(nbytes), 1)
    key = (device.index if device.index is not None else torch.cuda.current_device(),
           stream if stream is not None else torch.cuda.current_stream(device).cuda_stream)
    ws = _WS_CACHE.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
        _WS_CACHE[key] = ws
    return ws


def _fwd_workspace(lib, B, N, d, C, device, stream, ws=None, own=False):
    """(buffer, bytes to name in the call) of a forward call of this shape (d: of the padded queries): the cached buffer of
    the device and stream, or the caller's ``ws`` (``own``: always theirs, None at first), replaced when too small."""
    need = _fwd_ws_bytes(lib, B, N, d, C)
    if ws is None and not own:
        return _workspace(need, device, stream), need
    if ws is None or ws.numel() < max(need, 1):
        ws = torch.empty(max(need, 1), dtype=torch.uint8, device=device)
    return ws, ws.numel()


def nw_scores(q, s, kind="euclidean", logit_scale=None, support_cache=None):
    """q:(B,d), s:(N,d)|(B,N,d) -> (B,N) fp32 scores.  Replaces nwhead/kernel.py:13-44.
    support_cache: the SplitBank of `s` (a resident bank, e.g. the neighbour search over precompute()'s features): a bank
    that serves `s` with split rows as they stand (SplitBank, "scores") gives the scores from the split-fp16 tile kernel
    (the forward with its score output; 2-3x the fp32 scores kernel) when N is a multiple of 4."""
    _need_hip(q, s, logit_scale)
    lib = _lib.load()
    q, s = _f32c(q), _f32c(s)
    B, d = q.shape
    batched = s.dim() == 3
    N = s.shape[-2]
    out = torch.empty(B, N, dtype=torch.float32, device=q.device)
    ls = None if logit_scale is None else _f32c(logit_scale)
    bank_route = support_cache is not None and not batched and B > 0 and N > 0 and N % 4 == 0 and support_cache.matches(s)
    call = _resolve_scores(support_cache, q, s) if bank_route else None
    if call is not None:
        # one class, all labels 0: the aggregation is a formality, the (B, N) score matrix is what is wanted
        out1 = torch.empty(B, 1, dtype=torch.float32, device=q.device)
        st, d = _stream(q), call.q.shape[1]
        ws, ws_bytes = _fwd_workspace(lib, B, N, d, 1, q.device, st)
        with _OnDevice(q.device):
            _lib.check(lib.nw_fwd_f32(_ptr(call.q), _ptr(call.s), _ptr(call.sy), _ptr(call.norm2), _ptr(call.operand),
                                      _ptr(call.scale), _ptr(out1), _ptr(out), None, None, _ptr(ws), ws_bytes,
                                      B, N, d, 1, _kind_id(kind), _ptr(ls), 0, 0, call.opts, st), "nw_fwd_f32")
        return out
    with _OnDevice(q.device):
        _lib.check(lib.nw_scores_f32(_ptr(q), _ptr(s), _ptr(out), B, N, d, _kind_id(kind), _ptr(ls),
                                     int(batched), _stream(q)), "nw_scores_f32")
    return out


def nw_topk(scores, k, return_values=False):
    """scores (B,N) fp32 HIP tensor -> (B,k) int64 column indices, best score first, ties by ascending
    index: the first k columns of argsort(scores, descending=True, stable=True) (nwhead/utils.py:185-193),
    without sorting the other N-k.  k <= min(N, 1024)."""
    _need_hip(scores)
    lib = _lib.load()
    sc = _f32c(scores)
    B, N = sc.shape
    k = int(k)
    idx = torch.empty(B, k, dtype=torch.int64, device=sc.device)
    vals = torch.empty(B, k, dtype=torch.float32, device=sc.device) if return_values else None
    with _OnDevice(sc.device):
        _lib.check(lib.nw_topk_f32(_ptr(sc), _ptr(idx), _ptr(vals), B, N, k, _stream(sc)), "nw_topk_f32")
    return (idx, vals) if return_values else idx


KNN_FUSED_MIN_SCORE_BYTES = 1 << 30


def knn_fused_pays(B, N):
    """Whether the callers that used to go through the score matrix (KNN.indices, NWNet.get_neighbors) take nw_knn for B
    queries against N rows: from a (B, N) fp32 score matrix of KNN_FUSED_MIN_SCORE_BYTES on."""
    return 4 * int(B) * int(N) >= KNN_FUSED_MIN_SCORE_BYTES


def _row_window(row_window, B, device):
    """nw_knn's ``row_window`` as two contiguous (B,) int32 tensors."""
    if not isinstance(row_window, (tuple, list)) or len(row_window) != 2:
        raise ValueError("nw_knn: row_window is a pair (lo, hi) of (B,) integer tensors")
    out = []
    for t in row_window:
        if not torch.is_tensor(t) or t.is_floating_point() or t.is_complex() or t.dtype == torch.bool:
            raise ValueError("nw_knn: row_window holds integer tensors (bank rows)")
        if t.shape != (B,):
            raise ValueError(f"nw_knn: row_window tensors must be ({B},), one window per query; got {tuple(t.shape)}")
        if t.device != device:
            raise ValueError("nw_knn: row_window tensors must be on the queries' device")
        out.append(t.detach().to(torch.int32).contiguous())
    return out


def _masked_topk(scores, k, lo, hi, exclude, return_values):
    """nw_topk over the rows that a window admits, from the (B,N) score matrix; the slots past a query's valid count are
    (-1, -inf)."""
    N = scores.shape[1]
    cols = torch.arange(N, device=scores.device)
    keep = (cols >= lo[:, None]) & (cols < hi[:, None])
    if exclude:
        keep = ~keep
    idx, vals = nw_topk(scores.masked_fill(~keep, float("-inf")), k, return_values=True)
    empty = torch.arange(k, device=scores.device)[None, :] >= keep.sum(1)[:, None]
    idx = idx.masked_fill(empty, -1)
    return (idx, vals.masked_fill(empty, float("-inf"))) if return_values else idx


def nw_knn(q, bank, k, kind="euclidean", logit_scale=None, return_values=False, support=None, rounded=False,
           persistent_wgs=0, row_window=None, exclude=False):
    """q:(B,d), bank: the SplitBank of an (N,d) support -> (B,k) int64 rows of the tensor the bank was prepared from, best
    score first, equal scores in ascending row order (with return_values: also their (B,k) scores).  The neighbour search
    of nwhead/utils.py:185-193 and nwhead/nw.py:245-249 over a resident bank WITHOUT the (B,N) score matrix: the tiles of
    the split-fp16 kernel select their k best scores themselves (nw_knn_f32).

    The result is that of ``nw_topk(nw_scores(q, support, kind, logit_scale, support_cache=bank), k)``, and that route is
    taken as it stands -- it needs ``support``, the tensor the bank was prepared from -- when
    the bank has no split rows (a norms-only or fp16 bank), holds a class-sorted copy (built from unsorted labels), when
    k > 32, and for shapes whose bank-route scores come from the fp32 tile kernel (below 2e8 multiply-adds, unless
    NW_SPLIT_ALWAYS=1): the rows and values are the same either way.  (A bank whose N is no multiple of 4 has no
    bank-route scores; its fused search ranks the split kernel's scores, which lie within the same 3e-5 of the exact ones.)

    ``rounded=True`` (not the default, which it leaves as it is bit for bit): the exact search over the fp16-ROUNDED
    features of a ``precision="fp16"`` bank (nw_knn_f16) -- per query the k <= 32 rows with the largest score between the
    rounded query and the rounded rows (the rounding of nw_pack_rows_f16), computed in fp32 from ``bank.packed`` on the
    persistent 256-query kernel that serves 'full' inference from such a bank: half the bank bytes and a third of the
    matrix work of the split-row search, no score matrix, no second bank.  Order: score descending, equal fp32 scores by
    ascending row; the values returned are the very floats that were ranked.  Not bit-equal to any other route; the same
    bits from call to call and for every ``persistent_wgs`` (workgroups of the tile kernel, nw_fwd_opts.persistent_wgs).
    ``support`` is not needed.  Raises NWHipError when the bank cannot serve it: no packed rows (a bank of another
    precision, or a norms-only one of N <= 25), a class-sorted copy, k > 32, or queries whose width does not pad to the
    bank's.

    ``row_window=(lo, hi)`` (not the default, which it leaves as it is bit for bit): two (B,) integer tensors on the
    device; query b is searched over the rows lo[b] <= row < hi[b] only, or with ``exclude=True`` over every other row
    (lo >= hi: the empty window).  In a class-sorted bank that is "the supports of one class" / "of every other class",
    the leave-one-out search (window [i, i+1), excluded) or one segment of a concatenated bank.  The result is the k best
    rows the window admits, same scores and order as above; where it admits fewer than k, the remaining slots hold row -1
    and value -inf.  Where the search without a window is fused, this one is (nw_knn_window_f32: the window is applied in
    the tile epilogue); otherwise it masks the score matrix with torch ops and needs ``support``.  No window form of
    ``rounded=True`` exists: NWHipError."""
    _need_hip(q, logit_scale, support)
    if not isinstance(bank, SplitBank):
        raise TypeError("nw_knn searches a prepared bank: pass ops.SplitBank(support)")
    q = _f32c(q)
    B = q.shape[0]
    k = int(k)
    window = None
    if row_window is not None:
        if rounded:
            raise NWHipError("nw_knn(rounded=True): the rounded search has no window form (row_window needs the fp32 rows)")
        window = (*_row_window(row_window, B, q.device), exclude)
    N = bank.shape[0] if support is None or rounded else support.shape[-2]
    if not rounded and (k < 1 or k > N):
        raise NWHipError(f"nw_knn: k = {k} outside [1, N = {N}] (nw_topk refuses it too)")
    matches = None if support is None or rounded else support.dim() == 2 and N == bank.shape[0] and bank.matches(support)
    route = knn_route_for(bank, q.shape[1], B, k, matches, search_precision="fp16" if rounded else "fp32")
    if rounded and route != "rounded":
        raise NWHipError(f"nw_knn(rounded=True): {knn_rounded_refusal(bank, k, q.shape[1])}")
    if route == "matrix":
        if support is None:
            raise ValueError("nw_knn: this search goes through the score matrix and needs `support`, the tensor the bank was "
                             "prepared from")
        scores = nw_scores(q, support, kind, logit_scale, support_cache=bank)
        if window is not None:
            return _masked_topk(scores, k, *window, return_values)
        return nw_topk(scores, k, return_values=return_values)
    call = _resolve_scores(bank, q, rounded=rounded, persistent_wgs=persistent_wgs)
    return _knn_launch(call, N, k, kind, logit_scale, return_values, rounded, window)


def _knn_launch(call, N, k, kind, logit_scale, return_values, rounded, window):
    """The launch of a fused search over the operands of ``call`` (_resolve_scores): nw_knn_f16 (``rounded``),
    nw_knn_window_f32 (``window`` = (lo, hi, exclude)) or nw_knn_f32."""
    lib, q, (B, dp) = _lib.load(), call.q, call.q.shape
    ls = None if logit_scale is None else _f32c(logit_scale)
    idx = torch.empty(B, k, dtype=torch.int64, device=q.device)
    vals = torch.empty(B, k, dtype=torch.float32, device=q.device) if return_values else None
    if B == 0:
        return (idx, vals) if return_values else idx
    sizer = "nw_knn_f16_workspace_bytes" if rounded else "nw_knn_workspace_bytes"
    key = (sizer, B, N, dp, k)
    ws_bytes = _WS_BYTES.get(key)
    if ws_bytes is None:
        ws_bytes = _WS_BYTES[key] = getattr(lib, sizer)(B, N, dp, k)
    st = _stream(q)
    ws = _workspace(ws_bytes, q.device, st)
    operands = (_ptr(q), _ptr(call.operand), _ptr(call.scale), _ptr(call.norm2))
    rest = (_ptr(idx), _ptr(vals), _ptr(ws), ws_bytes, B, N, dp, k, _kind_id(kind), _ptr(ls))
    with _OnDevice(q.device):
        if rounded:
            _lib.check(lib.nw_knn_f16(*operands, *rest, call.opts, st), "nw_knn_f16")
        elif window is not None:
            lo, hi, exclude = window
            _lib.check(lib.nw_knn_window_f32(*operands, _ptr(lo), _ptr(hi), int(bool(exclude)), *rest, st), "nw_knn_window_f32")
        else:
            _lib.check(lib.nw_knn_f32(*operands, *rest, st), "nw_knn_f32")
    return (idx, vals) if return_values else idx


def _rounded_refusal(precision, packed, sorted_copy, shape, pad, k, width):
    N = shape[0]
    if precision != "fp16":
        return "the bank holds no fp16-packed rows (prepare it with precision='fp16')"
    if not packed:
        return f"a norms-only bank (N = {N} <= 25 rows: no tile kernel takes it)"
    if sorted_copy:
        return "the bank holds a class-sorted copy (it was built from unsorted labels): its rows are not the caller's"
    if k < 1 or k > N:
        return f"k = {k} outside [1, N = {N}]"
    if k > 32:
        return f"k = {k} > 32 (the tile epilogue's selection holds 32 keys per query)"
    if width is not None and width + pad != shape[1]:
        return f"queries of width {width} do not pad to the bank's width {shape[1]} (pad {pad})"
    return None


def knn_rounded_refusal(bank, k, width=None):
    """Why ``nw_knn(..., rounded=True)`` cannot search ``bank`` for k neighbours (queries of ``width`` columns), or None."""
    return _rounded_refusal(bank.precision, bank.packed is not None, bank.sorted_rows is not None, bank.shape, bank.pad, k, width)


def knn_route(*, precision, packed, split, sorted_copy, shape, pad, width, B, k, matches=None, search_precision="fp32",
              size_gate=False, need_n4=False, use_split=True):
    """Which search serves B queries of ``width`` columns for their k nearest rows of a prepared bank: the one rule of nw_knn
    and of the callers that choose between it and a search of their own (KNN.indices, NWNet.get_neighbors; a ShardedBank
    chooses nothing, it always calls nw_knn), over plain facts (no device, no bank object).  The bank: ``precision``,
    whether it holds ``packed`` (fp16) rows, ``split`` rows, a class-sorted copy, its ``shape`` (N, padded width) and ``pad``.
    ``matches``: whether the support tensor the caller names is the bank's (None: it names none).  ``use_split``: what
    nw_scores_use_split / force_split answer for the shape.  The caller's policy: ``search_precision``; ``size_gate``: k > 32
    and score matrices below KNN_FUSED_MIN_SCORE_BYTES stay the caller's own; ``need_n4``: so do banks with N % 4 != 0.
    -> "rounded" (nw_knn(rounded=True): nw_knn_f16), "fused" (nw_knn: nw_knn_f32 / nw_knn_window_f32), "matrix" (nw_knn ranks
    the bank route's score matrix with nw_topk) or None (the caller's gates keep the search: its own score matrix)."""
    N = shape[0]
    if search_precision == "fp16" and _rounded_refusal(precision, packed, sorted_copy, shape, pad, k, width) is None:
        return "rounded"
    if (size_gate and not (1 <= k <= 32 and knn_fused_pays(B, N))) or (need_n4 and N % 4):
        return None
    # the split rows are the caller's, the queries pad to them, and the scores nw_topk would rank are the split-row kernel's
    fused = (split and not sorted_copy and width + pad == shape[1] and matches is not False and 1 <= k <= 32 and N > 25
             and B > 0 and use_split)
    return "fused" if fused else "matrix"


def knn_route_for(bank, width, B, k, matches=None, **policy):
    """knn_route over the facts of ``bank`` (a SplitBank) and the library's size rule at its shape -- which is asked only
    where it decides: it turns "fused" into "matrix" and changes no other answer (a library call per search otherwise)."""
    route = knn_route(precision=bank.precision, packed=bank.packed is not None, split=bank.split is not None,
                      sorted_copy=bank.sorted_rows is not None, shape=bank.shape, pad=bank.pad, width=width, B=B, k=k,
                      matches=matches, **policy)
    if route == "fused" and not (_lib.force_split() or _lib.load().nw_scores_use_split(B, *bank.shape)):
        return "matrix"
    return route


HEAD_WINDOW_MAX_CLASSES = 160 * 1024 // 4 - 8     # the run merge's accumulators (fused_eligible)


def head_bank_refusal(*, split, sorted_copy, shape, pad, width, B, n_classes):
    """Why ``nw_head_bank`` cannot take nw_bwd_query_f32 for B queries of ``width`` columns over a prepared bank, over
    head_window_route's plain facts -- a sentence for the error text, or None when it can: the bank holds ``split`` rows
    that are the caller's (no class-sorted copy), the queries pad to its width, and the shape is one the kernel takes.
    The one statement of the regime of the head over a resident bank, forward and backward: head_window_route,
    head_weighted_route and head_bank_route read it."""
    N, d = shape
    if not split:
        return "the bank holds no split rows (a precision='fp16' or norms-only bank)"
    if sorted_copy:
        return "the bank was built from unsorted labels and keeps a class-sorted copy, whose rows are not the caller's"
    if width + pad != d:
        return f"queries of width {width} do not pad to the bank's width {d}"
    if N <= 25:
        return f"a bank of {N} rows is below the tile kernels (N > 25)"
    if d % 32 or not 32 <= d <= 1 << 20:
        return f"a bank of width {d} is not a multiple of 32 columns"
    if not 1 <= n_classes <= HEAD_WINDOW_MAX_CLASSES:
        return f"{n_classes} classes are outside [1, {HEAD_WINDOW_MAX_CLASSES}]"
    if B <= 0:
        return "an empty query batch"
    return None


def head_window_route(*, split, sorted_copy, shape, pad, width, B, n_classes):
    """Which route serves ``nw_head(..., row_window=...)`` for B queries of ``width`` columns over a prepared bank, over plain
    facts like knn_route: "fused" (nw_fwd_window_f32: the window is applied in the tile epilogue, no score matrix) at EVERY
    shape the kernel takes -- no size gate, the alternative is never the cheaper one -- that is whenever the bank holds
    ``split`` rows that are the caller's (no class-sorted copy), the queries pad to them (_resolve_scores' conditions) and
    N > 25; else "matrix" (nw_scores, a torch mask, nw_aggregate_f32): an fp16 or norms-only bank, a sorted copy, N <= 25."""
    return "fused" if head_bank_refusal(split=split, sorted_copy=sorted_copy, shape=shape, pad=pad, width=width, B=B,
                                        n_classes=n_classes) is None else "matrix"


def head_weighted_route(*, split, sorted_copy, shape, pad, width, B, n_classes, grad=False, grad_logw=False):
    """Which route serves a head with SUPPORT WEIGHTS (``row_logw``), beside head_window_route / head_bank_route and over the
    same plain facts: "fused" (nw_fwd_weighted_f32, and nw_bwd_query_weighted_f32 for the gradient: the weight is added in the
    tile epilogue, no score matrix) exactly when the windowed head would be fused -- both kernels take the same shapes, and
    the measured cost of the weights is N more floats per query tile, so there is no size gate either; else
    "matrix" for the forward (nw_scores + a (+ the window's mask) + nw_aggregate_f32, with the dead-query fix-up of
    nw_head_window).  The gradient (``grad``) has no matrix route that knows the weights -- nw_head's saves the scores its
    distance derivative is taken at, and they would be the weighted ones -- so it is None there, with a window or
    without: the caller refuses.  ``grad_logw`` -- the gradient to the WEIGHTS is wanted (nw_bwd_query_logw_f32, with or
    without ``grad`` for the queries) -- is served exactly where the query gradient is, "fused", and None elsewhere (an
    fp16 or norms-only bank, a class-sorted copy, N <= 25, a width that is no multiple of 32): the caller refuses and names
    nw_scores + a + nw_aggregate.  No size gate: at both shapes measured the fused weights-only step is faster than that
    composition and never holds a (B, N) buffer."""
    fused = head_window_route(split=split, sorted_copy=sorted_copy, shape=shape, pad=pad, width=width, B=B,
                              n_classes=n_classes) == "fused"
    return "fused" if fused else (None if (grad or grad_logw) else "matrix")


def _row_logw(row_logw, N, device, what):
    """``row_logw`` as the kernels read it: (N,) fp32, contiguous, 16-byte aligned, on ``device``.  No value is looked at."""
    if not torch.is_tensor(row_logw) or not row_logw.is_floating_point() or row_logw.shape != (N,):
        raise ValueError(f"{what}: row_logw is an ({N},) float tensor, the log-weight of every row of `s`")
    if row_logw.device != device:
        raise ValueError(f"{what}: row_logw must be on the queries' device")
    a = _f32c(row_logw.detach())
    return a if a.data_ptr() % 16 == 0 else a.clone()


def class_balance_logw(labels, n_classes, prior=None):
    """(N,) fp32 log-weights log(pi_c / n_c) for the rows of a bank with integer ``labels`` (N,): the weights of a class sum
    to its prior pi_c whatever its row count n_c, so an unbalanced bank predicts with that class prior -- flat (1 / C) by
    default, or ``prior`` (C,), positive entries.  Pass the result as ``row_logw`` / NWNet.set_support_weights.  Labels
    outside [0, n_classes) get -inf (the kernels skip such rows anyway); so do the rows of a class whose prior is 0."""
    C = int(n_classes)
    y = labels.detach().to(torch.int64)
    ok = (y >= 0) & (y < C)
    yc = y.clamp(0, max(C - 1, 0))
    counts = torch.bincount(yc[ok], minlength=C).to(torch.float64)
    pi = torch.full((C,), 1.0 / max(C, 1), dtype=torch.float64, device=y.device) if prior is None else \
        torch.as_tensor(prior, dtype=torch.float64, device=y.device)
    if pi.shape != (C,):
        raise ValueError(f"class_balance_logw: prior must be ({C},)")
    logw = (pi.log() - counts.clamp(min=1).log())[yc]
    return torch.where(ok, logw, logw.new_tensor(float("-inf"))).to(torch.float32)


KNN_MERGE_MAX_K, KNN_MERGE_MAX_SHARDS = 32, 64


def nw_knn_merge(vals, rows, labels, k, n_classes=None):
    """The cross-shard step of a neighbour search over a sharded bank (nw_knn_merge_f32): vals fp32 / rows int32 / labels
    int32, each (G, B, kc) -- per shard and query a list of kc candidates sorted best first, equal scores in ascending row
    order, rows < 0 marking "no element" -> ``(idx, vals, labels)``, each (B, k): the k best per query over all shards,
    score descending, equal scores by ascending (global) row; missing ones are (-1, -inf, -1).  With ``n_classes`` also the
    (B, C) log-probabilities of every query's own k neighbours (``nw_aggregate`` of the merged values and labels).

    The three inputs may be views into one gathered buffer: they need a unit stride inside a list, lists of a shard back to
    back, and one common stride between shards.  k <= kc <= 32, G <= 64."""
    _need_hip(vals, rows, labels)
    lib = _lib.load()
    if vals.dim() != 3 or rows.shape != vals.shape or labels.shape != vals.shape:
        raise ValueError("vals, rows and labels must be (G, B, kc) each")
    if vals.dtype != torch.float32 or rows.dtype != torch.int32 or labels.dtype != torch.int32:
        raise ValueError("vals must be float32, rows and labels int32")
    G, B, kc = vals.shape
    k = int(k)
    stride_g = vals.stride(0) if G > 1 else B * kc
    for t in (vals, rows, labels):
        if B * kc and (t.stride(2) != 1 or (B > 1 and t.stride(1) != kc) or (G > 1 and t.stride(0) != stride_g)):
            raise ValueError("nw_knn_merge: lists must be dense (B, kc) blocks with one common stride between shards")
    if k < 1 or k > KNN_MERGE_MAX_K or kc < k or kc > KNN_MERGE_MAX_K or G < 1 or G > KNN_MERGE_MAX_SHARDS:
        raise NWHipError(f"nw_knn_merge: needs 1 <= k <= kc <= {KNN_MERGE_MAX_K} and 1 <= G <= {KNN_MERGE_MAX_SHARDS} shards, "
                         f"got k = {k}, kc = {kc}, G = {G}")
    dev = vals.device
    C = 0 if n_classes is None else int(n_classes)
    idx = torch.empty(B, k, dtype=torch.int64, device=dev)
    val = torch.empty(B, k, dtype=torch.float32, device=dev)
    lab = torch.empty(B, k, dtype=torch.int64, device=dev)
    out = None if n_classes is None else torch.empty(B, C, dtype=torch.float32, device=dev)
    if B:
        with _OnDevice(dev):
            _lib.check(lib.nw_knn_merge_f32(_ptr(vals), _ptr(rows), _ptr(labels), G, B, kc, stride_g, k, C, _ptr(idx), _ptr(val),
                                            _ptr(lab), _ptr(out), _stream(vals)), "nw_knn_merge_f32")
    return (idx, val, lab) if n_classes is None else (idx, val, lab, out)


def row_norm2(x):
    """Squared L2 norm of every row of a (rows,d) fp32 HIP tensor -> (rows,).  Cache this for a support
    bank that does not change between calls and pass it as ``support_norm2``."""
    _need_hip(x)
    lib = _lib.load()
    xc = _f32c(x)
    out = torch.empty(xc.shape[0], dtype=torch.float32, device=xc.device)
    with _OnDevice(xc.device):
        _lib.check(lib.nw_row_norm2_f32(_ptr(xc), _ptr(out), xc.shape[0], xc.shape[1], _stream(xc)), "nw_row_norm2_f32")
    return out


def _check_label_range(lo, hi, n_classes=None, one_hot=False):
    """The range check of support labels, whose smallest / largest are ``lo`` / ``hi`` (None: not checked); the kernels
    would skip the others silently.  ``one_hot``: F.one_hot's own RuntimeError and messages (nw_head's validate_labels)."""
    err = RuntimeError if one_hot else ValueError
    if lo is not None and lo < 0:
        raise err("Class values must be non-negative." if one_hot else
                  "support labels must be non-negative class indices (F.one_hot, nw.py:276, raises too)")
    if n_classes is not None and hi is not None and hi >= int(n_classes):
        raise err("Class values must be smaller than num_classes." if one_hot else
                  f"support label {hi} is outside [0, n_classes={int(n_classes)}) (the reference's F.one_hot, nw.py:276, raises)")


class SplitBank:
    """A support matrix prepared once for repeated 'full' inference: split-fp16 rows, row scales and squared norms
    (nw_split_rows_f16x2).  Pass it as ``support_cache`` to the head entry points, or search it with nw_knn.
    The split format needs d % 32 == 0: a bank of another width (d >= 64) keeps a copy padded with zero columns
    (``rows``, ``pad``; no dot product or norm changes); narrower ones fall back to norms only (fp32 matrix cores).

    ``labels``: the (N,) labels that will be used with this bank.  The tile kernels sum softmax weights per RUN of equal
    consecutive labels, so a class-sorted bank (what precompute() builds) costs 1-2 sums per tile and an unsorted one a sum
    per row (measured 1862 vs 322 us at B=2048, N=50000).  The output does not depend on the order of the supports, so when
    unsorted labels are given the bank keeps a class-sorted copy (``sorted_rows`` / ``sorted_labels``, stable order).

    ``precision="fp16"``: the optional reduced-precision bank.  Instead of split rows it holds the rows ROUNDED to fp16
    with a power-of-two scale per row (nw_pack_rows_f16: ``packed``, ``packed_scale``, ``packed_norm2`` -- the norms of the
    rounded rows): half the bytes, one fp16 product per term instead of three; the head computed from them is the exact
    head of the rounded features (queries are rounded the same way inside the call; relative rounding 2^-11 per element).
    The width is zero-padded to max(192, next multiple of 64); ``split`` stays None and ``norm2`` holds the norms of the
    ORIGINAL rows.  A bank of 25 rows or fewer, which no tile kernel takes, keeps norms only.

    What a forward call hands to the library is decided in ONE place, _resolve, which every entry point calls, in this order:
    * class-sorted copy: it serves the call only when the caller passes the very label tensor the bank was sorted for (the
      same object, or the same address and shape), no output is indexed by support position (weights, influences, scores)
      and the support is not part of an autograd graph; otherwise the bank is dropped entirely, norms included (correct,
      slower).  (A caller that already passes the sorted copy is served as it stands.)
    * padded bank (``pad`` > 0): the queries are padded alike and the kernels read the bank's padded rows instead of the
      caller's tensor; of a support in an autograd graph only the norms are kept (the copy is not part of the graph).
    * nw_head pads queries and supports (torch ops) at d % 4 != 0, and training steps at d % 32 != 0 from d = 256 on (see
      _resolve), with or without a bank: a bank is then reduced to its norms.
    * operands: ``norm2`` with ``split`` / ``scale`` (none for a norms-only bank); the fp16 form (``packed*``,
      nw_fwd_opts.operand_form = 1) only where the call allows it -- no gradients, no weights, a shared support: training
      steps, weights, scores, influences and searches run on an fp16 bank as on a norms-only one.
    * scores (nw_scores' bank route, nw_knn's fused search; _resolve_scores): only split rows without a class-sorted copy.
    * the head over a row window (nw_head(row_window=...), nw_head_window; head_window_route): fused on the same terms as the
      scores -- split rows without a class-sorted copy, whose rows are the caller's -- else through the score matrix.
    * the head's query gradient over the bank as a constant (nw_head_bank; head_bank_route): fused on the same terms again,
      else nw_head's route without a window and a refusal with one.
    * the value head (nw_head_values, BankValues; head_values_route): fused on the same terms as the head over a row window,
      for values of 1 to 16384 columns, else through the score matrix, torch.softmax and a matmul.
    * searches, rounded (nw_knn(rounded=True); _resolve_scores): only fp16-packed rows without a class-sorted copy; the
      queries are padded to the bank's width like everywhere else.
    * run tables (build_tables): named in the call's options only when its labels are the tensor the tables were built
      from, unmodified; n_classes must then exceed every label of the tables.

    * the gradient to the bank rows (nw_head_bank(support_grad=True); head_bank_support_route): fused on the same terms as the
      query gradient, else nw_head's route without a window and weights and a refusal with either.
    * the value head's gradient to the bank rows (nw_head_values_bank(support_grad=True); head_values_grad_route): fused
      exactly where the value head is, else the matrix composition, windows and weights included.

    The bank's tensors are written again only by ``update_rows``, which replaces rows of the support and of every prepared
    form in place and keeps the bank matching its tensor, and by ``refresh``, which re-prepares every row in place after
    the support was written by something else (an optimizer step on learnable rows)."""

    def __init__(self, s, labels=None, precision="fp32"):
        if precision not in ("fp32", "fp16"):
            raise ValueError(f"precision must be 'fp32' or 'fp16', got {precision!r}")
        self.precision = precision
        _need_hip(s, labels)
        lib = _lib.load()
        sc = _f32c(s)
        # the tensor this bank was prepared from: identity, shape and in-place version (see matches())
        self._src = _sig(s)
        self.label_max = None
        if labels is not None and labels.numel():
            lo, hi = (int(v) for v in torch.aminmax(labels.detach()))
            _check_label_range(lo, None)
            self.label_max = hi                # nw_head refuses n_classes <= label_max, like F.one_hot
        self.pad, self.rows = 0, None
        half = precision == "fp16" and sc.dim() == 2 and sc.shape[0] > 25
        if half:
            self.pad = max(192, -(-sc.shape[1] // 64) * 64) - sc.shape[1]
            if self.pad:
                sc = self.rows = torch.nn.functional.pad(sc, (0, self.pad))
        elif precision == "fp32" and sc.dim() == 2 and sc.shape[1] % 32 and sc.shape[1] >= 64 and sc.shape[0] > 0:
            self.pad = (-sc.shape[1]) % 32
            sc = self.rows = torch.nn.functional.pad(sc, (0, self.pad))     # what the kernels read instead of `s`
        self.sorted_rows = self.sorted_labels = None
        if labels is not None and sc.dim() == 2 and labels.dim() == 1 and labels.numel() > 1:
            lab = labels.detach().to(torch.int64)
            if bool((lab[1:] < lab[:-1]).any()):
                perm = torch.argsort(lab, stable=True)
                self.sorted_rows, self.sorted_labels = sc[perm].contiguous(), lab[perm].contiguous()
                self._labels_ref = labels          # the label tensor this bank was sorted for (identity check only)
                sc = self.sorted_rows
        N, d = sc.shape
        self.shape = (N, d)
        self.split = self.scale = None
        self.packed = self.packed_scale = self.packed_norm2 = None
        if half:
            self.packed = torch.empty(N, d, dtype=torch.float16, device=sc.device)
            self.packed_scale = torch.empty(N, dtype=torch.float32, device=sc.device)
            self.packed_norm2 = torch.empty(N, dtype=torch.float32, device=sc.device)
            with _OnDevice(sc.device):
                _lib.check(lib.nw_pack_rows_f16(_ptr(sc), _ptr(self.packed), _ptr(self.packed_scale), _ptr(self.packed_norm2),
                                                N, d, _stream(sc)), "nw_pack_rows_f16")
            self.norm2 = row_norm2(sc)
        elif precision == "fp32" and d % 32 == 0 and N > 0:
            self.split = torch.empty_like(sc)
            self.scale = torch.empty(N, dtype=torch.float32, device=sc.device)
            self.norm2 = torch.empty(N, dtype=torch.float32, device=sc.device)
            with _OnDevice(sc.device):
                _lib.check(lib.nw_split_rows_f16x2(_ptr(sc), _ptr(self.split), _ptr(self.scale), _ptr(self.norm2),
                                                   N, d, _stream(sc)), "nw_split_rows_f16x2")
        else:
            self.norm2 = row_norm2(sc)
        self.tables = self._tables_src = None
        self.tables_label_max = -1
        self._opts, self._zero_labels = {}, None
        self.writes = 0        # update_rows calls so far (an autograd node that reads the bank in its backward checks it)
        if labels is not None and labels.dim() == 1 and self.has_operand_rows:
            self.build_tables(self.sorted_labels if self.sorted_labels is not None else labels)

    def update_rows(self, support, rows, x, momentum=0.0):
        """Replace rows of the bank IN PLACE (nw_bank_update_rows_f32, one launch): ``support`` -- the tensor this bank was
        prepared from -- gets ``x[i]`` in row ``rows[i]``, or with ``momentum`` in (0, 1) the blend
        ``momentum * old + (1 - momentum) * x[i]`` (every operation rounded in fp32), and every prepared form of those rows
        (fp32 rows of a padded bank, split rows and scales, norms, fp16-packed rows with their scales and norms) is left
        bit for bit as ``SplitBank(support, labels, precision)`` would build it from the updated tensor.  No other row is
        read or written, nothing is sorted, no host synchronisation; the labels, the run tables and the cached call options
        stay as they are (the labels of the rows do not change).

        rows: (R,) integer tensor on the device, R <= 16384; x: (R, support.shape[1]).  A row that is negative (the -1 of
        ``leave_out``) or past the bank is skipped; of several items naming one row the LAST wins and the others take no
        part.  The bank still ``matches(support)`` afterwards; ``support``'s in-place version is bumped, so autograd refuses
        a backward through a graph that saved it, and ``writes`` counts the call, which nw_head_bank's backward checks (it
        recomputes the scores from the bank).  Refused with NWHipError (bank_update_refusal): a bank built from unsorted
        labels, a norms-only bank, another feature width, R > 16384."""
        if not 0.0 <= float(momentum) < 1.0:
            raise ValueError(f"SplitBank.update_rows: momentum must be in [0, 1), got {momentum}")
        if not self.matches(support):
            raise ValueError("SplitBank.update_rows: `support` must be the tensor this bank was prepared from, unmodified since")
        _need_hip(support, rows, x)
        if x.dim() != 2 or rows.dim() != 1 or rows.shape[0] != x.shape[0] or rows.is_floating_point() or rows.dtype == torch.bool:
            raise ValueError("SplitBank.update_rows: rows is an (R,) integer tensor and x the (R, width) new rows")
        if support.dtype != torch.float32 or not support.is_contiguous():
            raise ValueError("SplitBank.update_rows writes into `support`: it must be a contiguous fp32 tensor")
        why = bank_update_refusal(split=self.split is not None, packed=self.packed is not None,
                                  sorted_copy=self.sorted_rows is not None, shape=self.shape, pad=self.pad, width=x.shape[1],
                                  R=x.shape[0])
        if why is not None:
            raise NWHipError(f"SplitBank.update_rows: {why}")
        xc = _f32c(x)
        if xc.untyped_storage().data_ptr() == support.untyped_storage().data_ptr():
            xc = xc.clone()            # (rows of the bank itself, e.g. support[perm]: read while they are written)
        rc = _i64c(rows.detach())
        N, d = self.shape
        padded = self.rows is not None
        s_rows = self.rows if padded else support.detach()
        with _OnDevice(support.device):
            _lib.check(_lib.load().nw_bank_update_rows_f32(
                _ptr(xc), _ptr(rc), xc.shape[0], xc.shape[1], float(momentum), _ptr(s_rows),
                _ptr(support.detach()) if padded else None, _ptr(self.norm2), _ptr(self.split), _ptr(self.scale),
                _ptr(self.packed), _ptr(self.packed_scale), _ptr(self.packed_norm2), N, d, _stream(support)),
                "nw_bank_update_rows_f32")
        if not support.is_inference():
            torch.autograd.graph.increment_version(support)
        self._src = _sig(support)
        self.writes += 1

    def refresh(self, support):
        """Re-prepare EVERY row of the bank from ``support`` IN PLACE, after something other than ``update_rows`` wrote the
        tensor (an optimizer step on learnable rows): the padded fp32 copy, split rows and scales, norms, fp16-packed rows with
        their scales and norms are written again into the buffers the bank already holds -- the launches of the constructor,
        so every prepared tensor is bit for bit what ``SplitBank(support, labels, precision)`` would build, at the same
        addresses and with no allocation (a ``support`` that is not contiguous fp32 is converted first, which allocates).
        ``support`` must have the shape and device the bank was prepared for; the bank ``matches`` it afterwards and
        ``writes`` counts the call (a pending nw_head_bank backward refuses, as after update_rows).  The labels, the run
        tables and the cached call options stay as they are.  Refused with NWHipError for a bank built from unsorted labels,
        whose class-sorted copy holds rows that are not the caller's."""
        _need_hip(support)
        if self.sorted_rows is not None:
            raise NWHipError("SplitBank.refresh: the bank was built from unsorted labels and keeps a class-sorted copy, whose "
                             "rows are not the caller's (build a new ops.SplitBank)")
        N, d = self.shape
        if support.dim() != 2 or tuple(support.shape) != (N, d - self.pad) or support.device != self.norm2.device:
            raise ValueError(f"SplitBank.refresh: `support` must be an ({N}, {d - self.pad}) tensor on the bank's device")
        lib = _lib.load()
        if self.rows is not None:
            self.rows[:, :d - self.pad].copy_(support.detach())      # (the zero columns stay)
            sc = self.rows
        else:
            sc = _f32c(support)
        with _OnDevice(sc.device):
            st = _stream(sc)
            if self.packed is not None:
                _lib.check(lib.nw_pack_rows_f16(_ptr(sc), _ptr(self.packed), _ptr(self.packed_scale), _ptr(self.packed_norm2),
                                                N, d, st), "nw_pack_rows_f16")
                _lib.check(lib.nw_row_norm2_f32(_ptr(sc), _ptr(self.norm2), N, d, st), "nw_row_norm2_f32")
            elif self.split is not None:
                _lib.check(lib.nw_split_rows_f16x2(_ptr(sc), _ptr(self.split), _ptr(self.scale), _ptr(self.norm2), N, d, st),
                           "nw_split_rows_f16x2")
            elif N > 0:
                _lib.check(lib.nw_row_norm2_f32(_ptr(sc), _ptr(self.norm2), N, d, st), "nw_row_norm2_f32")
        self._src = _sig(support)
        self.writes += 1

    @property
    def has_operand_rows(self):
        """Whether the bank holds split or fp16-packed rows (the banks that are given run tables when they are built)."""
        return self.split is not None or self.packed is not None

    def build_tables(self, labels):
        """Run tables of this bank under ``labels`` (nw_bank_tables_build): the forward then skips building them on
        every large launch.  They are used only for calls that pass this very label tensor, unmodified."""
        lib = _lib.load()
        lab64 = _i64c(labels.detach())
        N = self.shape[0]
        if lab64.dim() != 1 or lab64.numel() != N or N == 0 or not lab64.is_cuda:
            return
        lo, hi = (int(v) for v in torch.aminmax(lab64))
        _check_label_range(lo, None)
        self.tables_label_max = hi      # the tables hold every label as a real class: n_classes must exceed it (_call_opts)
        nbytes = lib.nw_bank_tables_bytes(N)
        tables = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=lab64.device)
        with _OnDevice(lab64.device):
            # C: any bound above the labels gives the same tables (nw_head refuses labels >= n_classes)
            _lib.check(lib.nw_bank_tables_build(_ptr(lab64), N, 0x7fffffff, _ptr(tables), nbytes, _stream(lab64)),
                       "nw_bank_tables_build")
        self.tables, self._tables_src, self._opts = tables, _sig(labels), {}

    def _call_opts(self, sy, sy_call, n_classes, persistent_wgs, operand_form):
        """Address of the nw_fwd_opts (kept alive in this bank) for a forward call with labels ``sy``, passed to the library
        as the int64 tensor ``sy_call``: names the cached run tables when ``sy`` is the label tensor they were built from
        (same storage, unmodified) -- the library uses them only for the address and row count of ``sy_call``."""
        if self.tables is None or _sig(sy) != self._tables_src:
            return _default_opts(persistent_wgs, operand_form)
        _check_label_range(None, self.tables_label_max, n_classes)
        key = (int(persistent_wgs), _lib.force_split(), sy_call.data_ptr(), sy_call.numel(), int(operand_form))
        op = self._opts.get(key)
        if op is None:
            if len(self._opts) > 64:
                self._opts.clear()
            op = self._opts[key] = _lib.fwd_opts(self.tables.data_ptr(), self.tables.numel(), persistent_wgs,
                                                 sy_call.data_ptr(), sy_call.numel(), operand_form)
        return C_addr(op)

    def matches(self, s):
        """True when `s` is the very tensor (storage, shape, no in-place update since) this bank was prepared from."""
        return _sig(s) == self._src


# What one forward call hands to the library (_resolve, _resolve_scores): the queries, padded where the rows are; the rows
# the kernel reads (None: a search, which reads only the operand); their int64 labels; squared row norms or None; the
# operand (split-fp16 rows, or fp16-packed rows when the options say operand_form = 1) with its row scales, or None; the
# address of the call's nw_fwd_opts.
_Call = collections.namedtuple("_Call", "q s sy norm2 operand scale opts")
_new_call = tuple.__new__    # (_Call(...) goes through a Python-level __new__: a third of a microsecond per forward)


def _pad_to_bank(bank, q, s):
    """Queries padded to the width of a padded bank, and the bank's padded rows in place of the caller's tensor."""
    return torch.nn.functional.pad(q, (0, bank.pad)), (bank.rows if s is not None and s.shape[-1] != bank.shape[1] else s)


def _resolve_scores(bank, q, s=None, rounded=False, persistent_wgs=0):
    """The _Call of a score call over the split rows of ``bank`` (rows `s`, one class, all labels zero), or of a search
    (no `s`, no labels); None when the bank cannot serve it as prepared (SplitBank's docstring, "scores").  ``rounded``: the
    search over the fp16-packed rows instead ("searches, rounded"), with ``persistent_wgs`` in its options."""
    if rounded:
        if bank.packed is None or bank.sorted_rows is not None or q.shape[1] + bank.pad != bank.shape[1]:
            return None
        if bank.pad:
            q, _ = _pad_to_bank(bank, q, None)
        return _new_call(_Call, (q, None, None, bank.packed_norm2, bank.packed, bank.packed_scale,
                                 _default_opts(persistent_wgs)))
    if bank.split is None or bank.sorted_rows is not None or q.shape[1] + bank.pad != bank.shape[1]:
        return None
    if bank.pad:
        q, s = _pad_to_bank(bank, q, s)
    sy = bank._zero_labels
    if sy is None and s is not None:
        sy = bank._zero_labels = torch.zeros(bank.shape[0], dtype=torch.int64, device=q.device)
    return _new_call(_Call, (q, s, sy, bank.norm2, bank.split, bank.scale, _default_opts()))


def _resolve(bank, q, s, sy, n_classes, positional=False, s_in_graph=False, half=False, persistent_wgs=0, norm2=None,
             torch_pad=None, run_tables=True):
    """The _Call of one forward (SplitBank's docstring has the rules).  ``bank``: the SplitBank of `s` or None; ``positional``:
    an output is indexed by support position; ``s_in_graph``: `s` is part of an autograd graph; ``half``: the fp16 operands
    may be used; ``norm2``: the caller's own norms; ``torch_pad``: nw_head's width rules (False: without, True: with a
    backward; None: no padding by torch ops); ``run_tables``: False for a call that never names them."""
    if bank is not None and bank.sorted_rows is not None and s.data_ptr() != bank.sorted_rows.data_ptr():
        ref = bank._labels_ref
        if positional or s_in_graph or not (sy is ref or (sy.data_ptr() == ref.data_ptr() and sy.shape == ref.shape)):
            bank = None
        else:
            s, sy = bank.sorted_rows, bank.sorted_labels
    if bank is not None and bank.pad:
        if s_in_graph:       # the padded copy is not part of the caller's graph
            norm2, bank = bank.norm2, None
        else:
            q, s = _pad_to_bank(bank, q, s)
    if torch_pad is not None and q.shape[-1] % 4 and s.dim() == 2 and s.shape[0] > 25:
        # an embedding size that is not a multiple of 4 would miss every tile kernel (they move 16-byte pieces) and land
        # on the generic two-kernel path (measured at d = 130: 925 us against 19 at d = 128; 52 ms with 20000 classes):
        # zero columns change no dot product and no norm, so the operands are padded (torch ops: autograd slices the
        # gradients back) and the cached norms, the bank's or the caller's, stay valid
        pad = (-q.shape[-1]) % 4
        if bank is not None:
            norm2, bank = bank.norm2, None
        q, s = torch.nn.functional.pad(q, (0, pad)), torch.nn.functional.pad(s, (0, pad))
    if torch_pad:
        _lib.sync_knobs()   # (NW_BWD_SPLIT and the other diagnostic switches may be flipped between steps)
        d = q.shape[-1]
        if (bank is None and s.dim() == 2 and d % 32 and d >= 256
                and _lib.load().nw_bwd_uses_split(q.shape[0], s.shape[0], d + (-d) % 32, int(n_classes), 0)):
            # a training step at a width that is not a multiple of 32: zero columns take it to the split-row kernels of the
            # forward and the backward (d = 1000 at T: 326 -> 237 us per eager forward + backward; narrow widths lose more to
            # the two extra torch ops than the kernels gain: d = 100, 168 -> 232 us); autograd slices the gradients back
            pad = (-d) % 32
            q, s = torch.nn.functional.pad(q, (0, pad)), torch.nn.functional.pad(s, (0, pad))
    syc = _i64c(sy)
    if bank is None:
        return _new_call(_Call, (q, s, syc, norm2, None, None, _default_opts(persistent_wgs)))
    norm2, operand, scale, form = bank.norm2, bank.split, bank.scale, 0
    if half and bank.packed is not None:       # an fp16 bank: the head of the rounded features
        if q.shape[1] != bank.shape[1]:
            raise ValueError(f"queries of width {q.shape[1]} against an fp16 bank of (padded) width {bank.shape[1]}")
        norm2, operand, scale, form = bank.packed_norm2, bank.packed, bank.packed_scale, 1
    opts = bank._call_opts(sy, syc, n_classes, persistent_wgs, form) if run_tables else _default_opts(persistent_wgs)
    return _new_call(_Call, (q, s, syc, norm2, operand, scale, opts))


class _NoCtx:
    """Stand-in for the autograd context on the inference path."""
    needs_input_grad = (False, False, False)

    @staticmethod
    def mark_non_differentiable(*a):
        pass


class _NWHeadFn(torch.autograd.Function):
    """autograd node for NWHead.forward (nwhead/nw.py:266-289)."""

    @staticmethod
    def forward(ctx, q, s, logit_scale, call, n_classes, kind_id, want_weights):
        """``call``: the _Call nw_head resolved; ``q`` / ``s`` are its queries and rows, as arguments of their own for autograd."""
        _, _, syc, sn2, ssplit, sscale, opts = call
        _need_hip(q, s, syc, logit_scale, sn2)
        lib = _lib.load()
        qc, sc = _f32c(q), _f32c(s)
        B, d = qc.shape
        sup_b = sc.dim() == 3
        lab_b = syc.dim() == 2
        N = sc.shape[-2]
        dev = qc.device
        need_bwd = any(ctx.needs_input_grad[:2]) or (logit_scale is not None and ctx.needs_input_grad[2])
        if need_bwd and ssplit is None and not sup_b and N > 0 and lib.nw_bwd_uses_split(B, N, d, n_classes, 0):
            # a training step at a size where the backward's products run on split rows: split the supports once,
            # for this forward (fp16 matrix cores instead of fp32) and for the backward
            ssplit, sscale = torch.empty_like(sc), torch.empty(N, dtype=torch.float32, device=dev)
            sn2 = torch.empty(N, dtype=torch.float32, device=dev)
            with _OnDevice(dev):
                _lib.check(lib.nw_split_rows_f16x2(_ptr(sc), _ptr(ssplit), _ptr(sscale), _ptr(sn2), N, d, _stream(qc)),
                           "nw_split_rows_f16x2")
        out = torch.empty(B, n_classes, dtype=torch.float32, device=dev)
        scores = torch.empty(B, N, dtype=torch.float32, device=dev) if need_bwd else None
        lse = torch.empty(B, dtype=torch.float32, device=dev) if need_bwd else None
        weights = torch.empty(B, N, dtype=torch.float32, device=dev) if want_weights else None
        ls = None if logit_scale is None else _f32c(logit_scale)
        st = _stream(qc)
        ws, ws_bytes = _fwd_workspace(lib, B, N, d, n_classes, dev, st)
        with _OnDevice(dev):
            rc = lib.nw_fwd_f32(_ptr(qc), _ptr(sc), _ptr(syc), _ptr(sn2), _ptr(ssplit), _ptr(sscale), _ptr(out),
                                _ptr(scores), _ptr(lse), _ptr(weights), _ptr(ws), ws_bytes, B, N, d, n_classes, kind_id,
                                _ptr(ls), int(sup_b), int(lab_b), opts, st)
        if rc:
            _lib.check(rc, "nw_fwd_f32")
        if need_bwd:
            ctx.save_for_backward(qc, sc, syc, scores, lse, out, ls if ls is not None else torch.empty(0, device=dev))
            ctx.meta = (B, N, d, n_classes, kind_id, sup_b, lab_b, ls is not None)
            # the bank of these supports, if there is one (SplitBank.update_rows writes it in place, but bumps the version
            # of the support saved above: autograd then refuses this backward)
            ctx.bank = (sn2, ssplit, sscale) if (ssplit is not None and not sup_b) else (None, None, None)
        if want_weights:
            ctx.mark_non_differentiable(weights)
            return out, weights
        return out

    @staticmethod
    def backward(ctx, gout, *unused):
        lib = _lib.load()
        qc, sc, syc, scores, lse, out, ls = ctx.saved_tensors
        B, N, d, C, kind_id, sup_b, lab_b, has_ls = ctx.meta
        dev = qc.device
        g = _f32c(gout)
        gq = torch.empty_like(qc)
        gs = torch.empty_like(sc)
        gls = torch.empty((), dtype=torch.float32, device=dev) if has_ls else None
        ws_bytes = lib.nw_bwd_workspace_bytes(B, N, d, C, kind_id, int(sup_b))
        ws = _workspace(ws_bytes, dev)
        bn2, bsplit, bscale = ctx.bank
        with _OnDevice(dev):
            _lib.check(lib.nw_bwd_bank_f32(_ptr(qc), _ptr(sc), _ptr(bn2), _ptr(bsplit), _ptr(bscale), _ptr(syc),
                                           _ptr(scores), _ptr(lse), _ptr(out),
                                           _ptr(g), _ptr(gq), _ptr(gs), _ptr(gls), _ptr(ws), ws_bytes,
                                           B, N, d, C, kind_id, _ptr(ls) if has_ls else None,
                                           int(sup_b), int(lab_b), _stream(qc)), "nw_bwd_bank_f32")
        return gq, gs, gls, None, None, None, None


def nw_head(q, s, sy, n_classes, kind="euclidean", logit_scale=None, return_weights=False,
            support_norm2=None, support_cache=None, validate_labels=False, row_window=None, exclude=False, row_logw=None):
    """NWHead.forward(x, sx, sy) -> (B,C) log-probs (and the (B,N) softmax weights on request).
    row_window=(lo, hi) (not the default, which it leaves as it is bit for bit; needs ``support_cache``, inference only):
    the head of query b over the rows lo[b] <= row < hi[b] of `s` alone, or with ``exclude=True`` over every other row --
    nw_head_window, which says more.
    row_logw (same conditions; ``None`` leaves every call as it is): (N,) float log-weights of the rows of `s`, added to the
    scores before the softmax; -inf removes a row.  nw_head_window says more; nw_head_bank is the call with gradients.
    support_norm2: optional cached ``row_norm2(s)`` for a shared (N,d) support.
    support_cache: optional ``SplitBank(s)`` (the fast 'full' inference path; its docstring says what the call then reads).
    validate_labels: the reference's F.one_hot (nw.py:276) REFUSES labels outside [0, n_classes); the kernels skip such
    supports silently (banks with labels check once, when they are built).  True: check here and raise F.one_hot's
    RuntimeError -- one device round trip per call, which is why it is opt-in (NWHead.validate_labels; NWNet's debug_mode
    turns it on)."""
    if validate_labels and sy.numel():
        _check_label_range(*(int(v) for v in torch.aminmax(sy.detach())), n_classes, one_hot=True)
    kid = _kind_id(kind)
    if kid == SCORE_KINDS["clip"] and logit_scale is None:
        raise ValueError("clip kernel needs logit_scale")
    if s.dim() == 2 and sy.dim() != 1 or s.dim() == 3 and sy.dim() != 2:
        raise ValueError("support labels must be (N,) for (N,d) supports and (B,N) for (B,N,d)")
    if support_norm2 is not None:
        if s.dim() != 2 or support_norm2.shape != (s.shape[0],):
            raise ValueError("support_norm2 must be (N,) for an (N,d) support")
        support_norm2 = _f32c(support_norm2)
    if support_cache is not None:
        if s.dim() != 2 or not support_cache.matches(s):
            raise ValueError("support_cache was prepared from another support tensor (or the tensor was modified in place "
                             "since): build a new ops.SplitBank(s) -- the split rows and norms it holds are those of the "
                             "tensor it was built from")
        _check_label_range(None, support_cache.label_max, n_classes)
    grad = torch.is_grad_enabled()
    needs_grad = grad and (q.requires_grad or s.requires_grad or (logit_scale is not None and logit_scale.requires_grad))
    if row_window is not None or row_logw is not None:
        if needs_grad or return_weights or support_cache is None:
            raise ValueError("nw_head(row_window=... / row_logw=...) is inference over a prepared bank: it needs support_cache "
                             "and has no gradients (nw_head_bank has the queries') and no return_weights")
        return nw_head_window(q, s, sy, n_classes, support_cache, row_window, exclude, kind, logit_scale, row_logw=row_logw)
    call = _resolve(support_cache, q, s, sy, n_classes, return_weights, grad and s.requires_grad,
                    not (needs_grad or return_weights), 0, support_norm2, needs_grad)      # (by position: host-bound)
    if not needs_grad:   # inference: skip the autograd node (its bookkeeping costs more than the kernels at small sizes)
        return _NWHeadFn.forward(_NoCtx, call.q, call.s, logit_scale, call, int(n_classes), kid, bool(return_weights))
    return _NWHeadFn.apply(call.q, call.s, logit_scale, call, int(n_classes), kid, bool(return_weights))


def _window_empty(lo, hi, exclude, N):
    """(B,) bool: the queries whose window admits no row of an N-row bank (lo / hi clamped to [0, N] like the kernel does)."""
    lo, hi = lo.clamp(0, N), hi.clamp(0, N)
    return ((lo <= 0) & (hi >= N)) if exclude else (hi <= lo)


def _bank_head_fwd(q, call, syc, logw, lo, hi, exclude, out, lse, kind_id, ls):
    """The one launch of the head over a resident bank with a row window, support weights or both, into ``out`` / ``lse``:
    nw_fwd_window_f32 without weights (``logw`` None), nw_fwd_weighted_f32 with them.  ``q``: the fp32 queries padded to the
    bank, ``call``: the _Call of its split rows (_resolve_scores), ``syc``: int64 labels, ``lo`` / ``hi``: int32 or None."""
    lib = _lib.load()
    (B, d), N, C, st = q.shape, call.operand.shape[0], out.shape[1], _stream(q)
    ws, ws_bytes = _fwd_workspace(lib, B, N, d, C, q.device, st)
    entry = "nw_fwd_window_f32" if logw is None else "nw_fwd_weighted_f32"
    with _OnDevice(q.device):
        _lib.check(getattr(lib, entry)(_ptr(q), _ptr(call.operand), _ptr(call.scale), _ptr(call.norm2), _ptr(syc),
                                       *(() if logw is None else (_ptr(logw),)), _ptr(lo), _ptr(hi), int(bool(exclude)),
                                       _ptr(out), _ptr(lse), _ptr(ws), ws_bytes, B, N, d, C, kind_id, _ptr(ls), st), entry)


def _bank_head_bwd(q, operands, logw, lo, hi, exclude, lse, out, gout, kind_id, ls, want_gq=True, want_glogw=False):
    """The one launch of the gradients of that head -> (gq, glogit_scale, glogw), None where not asked for (glogit_scale:
    whenever there is a clip scale ``ls``).  nw_bwd_query_f32 without weights, nw_bwd_query_weighted_f32 with constant ones,
    nw_bwd_query_logw_f32 with its own workspace size when their gradient is wanted (``want_glogw``; gq is then optional).
    ``operands``: the bank's (split, scale, norm2) and the int64 labels, as the forward read them."""
    lib = _lib.load()
    ssplit, sscale, sn2, syc = operands
    (B, d), N, C, dev = q.shape, ssplit.shape[0], out.shape[1], q.device
    gq = torch.empty_like(q) if want_gq else None
    gls = torch.empty((), dtype=torch.float32, device=dev) if ls is not None else None
    glogw = torch.empty(N, dtype=torch.float32, device=dev) if want_glogw else None
    if want_glogw:
        entry, ws_bytes = "nw_bwd_query_logw_f32", lib.nw_bwd_logw_workspace_bytes(B, N, d, C, 0, int(want_gq))
    else:
        entry = "nw_bwd_query_f32" if logw is None else "nw_bwd_query_weighted_f32"
        ws_bytes = lib.nw_bwd_query_workspace_bytes(B, N, d, C, 0)
    ws = _workspace(ws_bytes, dev)
    with _OnDevice(dev):
        _lib.check(getattr(lib, entry)(_ptr(q), _ptr(ssplit), _ptr(sscale), _ptr(sn2), _ptr(syc),
                                       *(() if logw is None else (_ptr(logw),)), _ptr(lo), _ptr(hi), int(exclude), _ptr(lse),
                                       _ptr(out), _ptr(gout), _ptr(gq), *((_ptr(glogw),) if want_glogw else ()), _ptr(gls),
                                       _ptr(ws), ws_bytes, B, N, d, C, kind_id, _ptr(ls), 0, _stream(q)), entry)
    return gq, gls, glogw


def nw_head_window(q, s, sy, n_classes, bank, row_window, exclude=False, kind="euclidean", logit_scale=None, return_lse=False,
                   row_logw=None):
    """``nw_head(q, s, sy, n_classes, support_cache=bank, row_window=(lo, hi), exclude=...)``: the head of every query over
    its own ROW WINDOW of the bank -> (B,C) log-probs (with ``return_lse`` also the (B,) log-sum-exp of the admitted scores).
    lo / hi: (B,) integer tensors on the device, rows of `s`, the tensor the bank was prepared from; query b sees the rows
    lo[b] <= row < hi[b] only, or with ``exclude`` every other row (lo >= hi: the empty window; values are clamped to
    [0, N]).  Leave-one-out prediction of bank rows is the window [i, i+1), excluded; one environment of a concatenated bank
    or one class of a class-sorted one is a kept window, "every other" the same window excluded.  The softmax runs over the
    admitted rows alone -- the window is applied to the scores before the maximum and the exponentials, so an excluded row
    that would dominate the full softmax (a query's own copy in the bank, at distance 0) leaves no trace.  A query whose
    window admits no row gets log(1e-12) in every class and lse = -inf.  Inference only.

    Route (head_window_route): nw_fwd_window_f32 -- the split-fp16 tile kernel with the window in its epilogue, no (B,N)
    matrix -- at every shape the kernel takes, whenever the bank holds split rows without a class-sorted copy and the
    queries pad to its width; otherwise (a ``precision="fp16"`` or norms-only bank, a bank built from unsorted labels,
    N <= 25) nw_scores over the bank, a torch mask and nw_aggregate_f32: the same result through the (B,N) score matrix.

    row_logw: SUPPORT WEIGHTS, (N,) float log-weights a_j = log w_j of the rows of `s` (``row_window`` may then be None: no
    window).  The head becomes log(sum_{j admitted, y_j = c} w_j e^score / sum_{j admitted} w_j e^score + 1e-12): the head of
    score + a.  a_j = -inf removes row j (soft deletion, any subset of a live bank), ops.class_balance_logw gives an unbalanced
    bank a flat class prior, anything finite is an importance weight.  Values must be finite or -inf; NaN, +inf and magnitudes
    above ~1e38 / 1.45 are outside the contract (undefined results for the queries that admit such a row, no fault; nothing is
    checked here -- NWNet.set_support_weights checks once).  A query all of whose admitted rows have a = -inf is dead like one
    with an empty window.  Route (head_weighted_route): nw_fwd_weighted_f32 wherever the windowed head is fused, the weight
    added in the tile epilogue before the maximum; else nw_scores + a + the mask + nw_aggregate_f32."""
    _need_hip(q, s, sy, logit_scale)
    if not isinstance(bank, SplitBank):
        raise TypeError("nw_head_window runs over a prepared bank: pass ops.SplitBank(support)")
    if s.dim() != 2 or sy.dim() != 1 or sy.shape[0] != s.shape[0] or not bank.matches(s):
        raise ValueError("nw_head_window: `s` (N,d) must be the tensor the bank was prepared from and `sy` its (N,) labels")
    lib = _lib.load()
    q = _f32c(q)
    B, N, C = q.shape[0], s.shape[0], int(n_classes)
    if row_window is None and row_logw is None:
        raise ValueError("nw_head_window: needs row_window=(lo, hi), row_logw, or both")
    lo, hi = _row_window(row_window, B, q.device) if row_window is not None else (None, None)
    logw = None if row_logw is None else _row_logw(row_logw, N, q.device, "nw_head_window")
    ls = None if logit_scale is None else _f32c(logit_scale)
    kid = _kind_id(kind)
    if kid == SCORE_KINDS["clip"] and ls is None:
        raise ValueError("clip kernel needs logit_scale")
    syc = _i64c(sy)
    out = torch.empty(B, C, dtype=torch.float32, device=q.device)
    lse = torch.empty(B, dtype=torch.float32, device=q.device)
    facts = dict(split=bank.split is not None, sorted_copy=bank.sorted_rows is not None, shape=bank.shape, pad=bank.pad,
                 width=q.shape[1], B=B, n_classes=C)
    route = head_window_route(**facts) if logw is None else head_weighted_route(**facts)
    if route == "fused":
        call = _resolve_scores(bank, q)
        _bank_head_fwd(call.q, call, syc, logw, lo, hi, exclude, out, lse, kid, ls)
    elif B > 0:
        scores = nw_scores(q, s, kind, logit_scale, support_cache=bank)
        if logw is not None:
            scores += logw
        if lo is not None:
            cols = torch.arange(N, device=q.device)
            keep = (cols >= lo[:, None]) & (cols < hi[:, None])
            if exclude:
                keep = ~keep
            scores.masked_fill_(~keep, float("-inf"))
        with _OnDevice(q.device):
            _lib.check(lib.nw_aggregate_f32(_ptr(scores), _ptr(syc), _ptr(out), _ptr(lse), None, B, N, C, 0, _stream(q)),
                       "nw_aggregate_f32")
        # (a softmax over nothing: the kernel's answer is not defined)
        empty = _window_empty(lo, hi, exclude, N) if logw is None else ~(scores > float("-inf")).any(dim=1)
        out = torch.where(empty[:, None], out.new_tensor(1e-12).log(), out)
        lse = lse.masked_fill(empty, float("-inf"))
    return (out, lse) if return_lse else out


def head_bank_route(*, split, sorted_copy, shape, pad, width, B, n_classes):
    """Which route serves the gradients of ``nw_head_bank``, beside head_window_route and over the same facts: "fused"
    (nw_bwd_query_f32: scores recomputed tile by tile, no (B,N) buffer, no support gradient) whenever head_bank_refusal
    has nothing to say; else "matrix": nw_head's route through the score matrix without a window, a refusal with one."""
    return "fused" if head_bank_refusal(split=split, sorted_copy=sorted_copy, shape=shape, pad=pad, width=width, B=B,
                                        n_classes=n_classes) is None else "matrix"


def head_bank_support_route(*, split, sorted_copy, shape, pad, width, B, n_classes, window=False, weights=False):
    """Which route serves the gradient to the BANK ROWS of ``nw_head_bank(..., support_grad=True)``, beside head_bank_route
    and over the same plain facts (``window`` / ``weights``: the call has a row window / support weights): "fused"
    (nw_bwd_bank_support_f32: the coefficients recomputed tile by tile and contracted with the queries, no (B, N) buffer)
    whenever head_bank_refusal has nothing to say -- no size gate, the keyword is the caller's choice and the route is kept
    for its memory where it is the slower one; else "matrix", nw_head's route through the score matrix, which
    computes gs already, when the call has neither a window nor weights, and NWHipError with either: that route knows
    neither."""
    why = head_bank_refusal(split=split, sorted_copy=sorted_copy, shape=shape, pad=pad, width=width, B=B, n_classes=n_classes)
    if why is None:
        return "fused"
    if window or weights:
        what = "row_window" if window else "row_logw"
        raise NWHipError(f"nw_head_bank({what}=..., support_grad=True) has no gradient route here: {why}")
    return "matrix"


HEAD_VALUES_MAX_T = 16384        # nw_fwd_values_f32: value columns per row (after padding to a multiple of 32)


def head_values_route(*, split, sorted_copy, shape, pad, width, B, T):
    """Which route serves the VALUE head ``nw_head_values`` for B queries of ``width`` columns and values of ``T`` columns over
    a prepared bank, beside head_window_route and over the same plain facts: "fused" (the forward's lse pass, then
    nw_fwd_values_f32: no (B, N) matrix) exactly where head_bank_refusal is silent -- the bank holds split rows that are the
    caller's, the queries pad to its width, N > 25, B > 0 -- and 1 <= T <= HEAD_VALUES_MAX_T (the values pad to a multiple
    of 32 columns themselves); else "matrix": nw_scores over the bank, + row_logw, the window's mask, torch.softmax and a
    matmul with the values -- an fp16 or norms-only bank, a class-sorted copy, N <= 25, widths that do not pad.  No size
    gate: the matrix route holds the (B, N) matrix twice, which is the reason for the fused one at every shape it was timed
    at (DESIGN 4.8k has the times)."""
    fused = 1 <= T <= HEAD_VALUES_MAX_T and head_bank_refusal(split=split, sorted_copy=sorted_copy, shape=shape, pad=pad,
                                                              width=width, B=B, n_classes=1) is None
    return "fused" if fused else "matrix"


class BankValues:
    """Real-valued targets for the rows of a SplitBank, prepared once for ``nw_head_values``: ``values`` (N, T), any float
    dtype, row j the target of row j of the tensor ``bank`` was prepared from (regression targets, soft / smoothed / multi-hot
    labels, per-row attributes).  Keeps an fp32 copy zero-padded to a multiple of 32 columns (``rows``, (N, ``width``)) and
    its split-fp16 form (``split``, ``scale``: nw_split_rows_f16x2 over the padded copy, the norms dropped) -- 8 N width
    bytes; ``T`` is the caller's column count.  Every value must be FINITE, in every row (a row that a window or a -inf
    weight removes still meets the matrix pipe with a 0 coefficient, and 0 x inf is NaN); nothing is checked.  The split
    format scales by ROW: an element keeps 22 bits down to 2^-18 of its row's largest magnitude, an absolute error of 2^-38
    of that below -- columns of very different magnitude belong in separate BankValues.
    ``matches(values)``: the very tensor, not written since; ``stale()``: that tensor is alive and was written.  After such a write ``refresh()`` re-prepares in place from the live tensor (no
    allocation); there is no update of single value rows.  T above HEAD_VALUES_MAX_T keeps the fp32 copy only (the matrix route)."""

    def __init__(self, values, bank):
        if not isinstance(bank, SplitBank):
            raise TypeError("BankValues: `bank` is the ops.SplitBank whose rows the values belong to")
        if not torch.is_tensor(values) or not values.is_floating_point() or values.dim() != 2 or values.shape[1] < 1:
            raise ValueError("BankValues: values is an (N, T) float tensor, T >= 1: one target row per bank row")
        if values.shape[0] != bank.shape[0]:
            raise ValueError(f"BankValues: {values.shape[0]} value rows for a bank of {bank.shape[0]} rows")
        _need_hip(values)
        self._src, self._ref = _sig(values), weakref.ref(values)      # (no hold on the caller's tensor)
        self.requires_grad = bool(values.requires_grad)
        N, T = values.shape
        self.T, self.width = T, T + (-T) % 32
        vc = _f32c(values)
        self.rows = torch.nn.functional.pad(vc, (0, self.width - T)) if self.width != T else (vc.clone() if vc.data_ptr() == values.data_ptr() else vc)
        self.split = self.scale = None
        if N > 0 and self.width <= HEAD_VALUES_MAX_T:
            self.split = torch.empty_like(self.rows)
            self.scale = torch.empty(N, dtype=torch.float32, device=vc.device)
            norm2 = self._norm2 = torch.empty(N, dtype=torch.float32, device=vc.device)      # (the packer's third output: not needed)
            with _OnDevice(vc.device):
                _lib.check(_lib.load().nw_split_rows_f16x2(_ptr(self.rows), _ptr(self.split), _ptr(self.scale), _ptr(norm2),
                                                           N, self.width, _stream(vc)), "nw_split_rows_f16x2")

    def source(self):
        """The tensor this object was prepared from, or None when it is gone (only a weak reference is kept)."""
        return self._ref()

    def refresh(self):
        """Re-prepare IN PLACE from the live source tensor after it was written (an optimiser step on learnable values): the
        copy into the padded fp32 rows and one nw_split_rows_f16x2 into the existing buffers -- no allocation -- and the
        staleness signature moves to the tensor's present version.  A training loop that steps the values calls this once
        per step instead of building a new BankValues.  The source gone: NWHipError."""
        t = self._ref()
        if t is None:
            raise NWHipError("BankValues.refresh: the tensor this object was prepared from is gone; build a new ops.BankValues")
        if t.data_ptr() != self._src[0] or tuple(t.shape) != self._src[1]:
            raise NWHipError("BankValues.refresh: the source tensor was replaced or reshaped; build a new ops.BankValues")
        with torch.no_grad():
            self.rows[:, :self.T].copy_(t.detach())
        if self.split is not None:
            with _OnDevice(self.rows.device):
                _lib.check(_lib.load().nw_split_rows_f16x2(_ptr(self.rows), _ptr(self.split), _ptr(self.scale), _ptr(self._norm2),
                                                           self.rows.shape[0], self.width, _stream(self.rows)),
                           "nw_split_rows_f16x2")
        self._src = _sig(t)
        self.requires_grad = bool(t.requires_grad)
        return self

    def matches(self, values):
        """True when ``values`` is the very tensor (storage, shape, no in-place update since) this object was prepared from."""
        return _sig(values) == self._src

    def stale(self):
        """True when the source tensor is still alive and was written in place since: what nw_head_values refuses."""
        t = self._ref()
        return t is not None and _sig(t) != self._src


def nw_head_values(q, s, bank, values, kind="euclidean", logit_scale=None, row_window=None, exclude=False, row_logw=None,
                   log=False, return_lse=False):
    """The VALUE head (Nadaraya-Watson regression) over a prepared bank: q (B,d), ``s`` (N,d) the tensor ``bank`` (a SplitBank)
    was prepared from, ``values`` the targets of its rows -> (B,T) fp32
        out[b] = sum_{j admitted} softmax_j(score_bj + a_j) values[j]
    (with ``return_lse`` also the (B,) log-sum-exp of the admitted weighted scores).  ``values``: a BankValues (prepared
    once), or a raw (N,T) float tensor, which is prepared on the fly -- an fp32 copy, the padding and one split launch over
    N x T values per call: prepare it once for repeated calls.  ``row_window`` / ``exclude`` / ``row_logw`` mean what they
    mean for nw_head_window: the softmax runs over the admitted rows alone (leave-one-out regression is the window
    [i, i+1), excluded), a_j = -inf removes a row.  Every value must be finite, in every row.  ``log``: log(out + 1e-12), for
    soft-label classification -- one-hot values of the labels reproduce nw_head_window.  A dead query (no admitted row)
    gets 0 in every column (``log``: log(1e-12)) and lse = -inf.

    Inference only: a ``q``, ``values`` or ``row_logw`` that requires grad while grad mode is enabled raises NWHipError --
    the differentiable route is the composition nw_scores + softmax + matmul (torch autograd); for the gradient to the
    queries alone, without a (B, N) matrix, nw_head_values_bank.

    Route (head_values_route): "fused" -- the forward's lse pass (nw_fwd_window_f32 / nw_fwd_weighted_f32 over all-zero
    labels, one class, the kept window [0, N) when there is none) and nw_fwd_values_f32, no (B,N) matrix -- wherever the
    windowed head is fused and T <= 16384; else "matrix": nw_scores, + row_logw, the mask, torch.softmax, @ values.  A
    BankValues whose tensor was written since it was prepared is REFUSED (ValueError), not rebuilt."""
    _need_hip(q, s, logit_scale)
    if not isinstance(bank, SplitBank):
        raise TypeError("nw_head_values runs over a prepared bank: pass ops.SplitBank(support)")
    if s.dim() != 2 or not bank.matches(s):
        raise ValueError("nw_head_values: `s` (N,d) must be the tensor the bank was prepared from")
    raw = values if torch.is_tensor(values) else None
    if torch.is_grad_enabled() and (q.requires_grad or (raw.requires_grad if raw is not None else getattr(values, "requires_grad", False))
                                    or (torch.is_tensor(row_logw) and row_logw.requires_grad)):
        raise NWHipError("nw_head_values is inference only and does not detach silently: q, values or row_logw requires grad. "
                         "The differentiable route is the composition nw_scores + softmax + matmul")
    if raw is not None:
        values = BankValues(raw, bank)
    elif not isinstance(values, BankValues):
        raise TypeError("nw_head_values: values is an ops.BankValues or an (N,T) float tensor")
    N, T = s.shape[0], values.T
    if values.rows.shape[0] != N or values.rows.device != q.device:
        raise ValueError(f"nw_head_values: the values hold {values.rows.shape[0]} rows on {values.rows.device} for a bank of {N} "
                         f"rows and queries on {q.device}")
    if values.stale():
        raise ValueError("nw_head_values: the tensor this BankValues was prepared from was written since; build a new "
                         "ops.BankValues")
    q = _f32c(q)
    if q.data_ptr() % 16:
        q = q.clone()
    B = q.shape[0]
    lo, hi = _row_window(row_window, B, q.device) if row_window is not None else (None, None)
    logw = None if row_logw is None else _row_logw(row_logw, N, q.device, "nw_head_values")
    ls = None if logit_scale is None else _f32c(logit_scale)
    kid = _kind_id(kind)
    if kid == SCORE_KINDS["clip"] and ls is None:
        raise ValueError("clip kernel needs logit_scale")
    route = head_values_route(split=bank.split is not None, sorted_copy=bank.sorted_rows is not None, shape=bank.shape,
                              pad=bank.pad, width=q.shape[1], B=B, T=T)
    if route == "fused":
        out, lse = _values_head_fwd(_resolve_scores(bank, q, s), bank, values, logw, lo, hi, exclude, kid, ls)
        if values.width != T:
            out = out[:, :T]
    else:
        vals = values.rows[:, :T]
        if B == 0 or N == 0:
            out = torch.zeros(B, T, dtype=torch.float32, device=q.device)
            lse = torch.full((B,), float("-inf"), dtype=torch.float32, device=q.device)
        else:
            scores = nw_scores(q, s, kind, logit_scale, support_cache=bank)
            if logw is not None:
                scores += logw
            if lo is not None:
                cols = torch.arange(N, device=q.device)
                keep = (cols >= lo[:, None]) & (cols < hi[:, None])
                if exclude:
                    keep = ~keep
                scores.masked_fill_(~keep, float("-inf"))
            # (a softmax over nothing is NaN: a dead query gets weight 0 in every row)
            dead = ~(scores > float("-inf")).any(dim=1)
            lse = torch.logsumexp(scores, dim=1).masked_fill(dead, float("-inf"))
            out = torch.softmax(scores, dim=1).masked_fill(dead[:, None], 0.0) @ vals
    if log:
        out = torch.log(out + 1e-12)
    elif not out.is_contiguous():
        out = out.contiguous()
    return (out, lse) if return_lse else out


def _values_head_fwd(call, bank, values, logw, lo, hi, exclude, kind_id, ls):
    """The two launches of the fused value head -> (out (B, values.width), lse (B,)): the forward's lse pass (_bank_head_fwd
    over all-zero labels and one class; the kept window [0, N) when there is neither a window nor weights), then
    nw_fwd_values_f32.  ``call``: _resolve_scores' _Call of the fp32 queries padded to the bank (``call.q``)."""
    lib = _lib.load()
    qp, N, Tp = call.q, call.operand.shape[0], values.width
    (B, d), dev, st = qp.shape, qp.device, _stream(qp)
    lse = torch.empty(B, dtype=torch.float32, device=dev)
    out1 = torch.empty(B, 1, dtype=torch.float32, device=dev)
    flo, fhi = (lo, hi) if lo is not None or logw is not None else _whole_window(bank, B, N, dev)
    _bank_head_fwd(qp, call, call.sy, logw, flo, fhi, exclude and lo is not None, out1, lse, kind_id, ls)
    out = torch.empty(B, Tp, dtype=torch.float32, device=dev)
    ws_bytes = lib.nw_fwd_values_workspace_bytes(B, N, d, Tp, 0)
    ws = _workspace(ws_bytes, dev, st)
    with _OnDevice(dev):
        _lib.check(lib.nw_fwd_values_f32(_ptr(qp), _ptr(call.operand), _ptr(call.scale), _ptr(call.norm2), _ptr(values.split),
                                         _ptr(values.scale), _ptr(logw), _ptr(lo), _ptr(hi), int(bool(exclude)), _ptr(lse),
                                         _ptr(out), _ptr(ws), ws_bytes, B, N, d, Tp, kind_id, _ptr(ls), 0, st), "nw_fwd_values_f32")
    return out, lse


def _whole_window(bank, B, N, device):
    """The kept window [0, N) of B queries as two (B,) int32 tensors, cached on the bank (the lse pass of a value head
    without a window or weights goes through nw_fwd_window_f32, which wants one)."""
    cached = getattr(bank, "_whole", None)
    if cached is None or cached[0].shape[0] != B or cached[0].device != device:
        cached = bank._whole = (torch.zeros(B, dtype=torch.int32, device=device),
                                torch.full((B,), N, dtype=torch.int32, device=device))
    return cached


BANK_UPDATE_MAX_ROWS = 16384     # nw_bank_update_rows_f32: every wave scans the rest of `rows` for its own row


def bank_update_refusal(*, split, packed, sorted_copy, shape, pad, width, R):
    """Why ``SplitBank.update_rows`` cannot write R new rows of ``width`` columns into a prepared bank, over the plain
    facts of the bank -- a sentence for the error text, or None when it can: the bank's rows are the caller's (no
    class-sorted copy), it holds ``split`` or fp16-``packed`` rows, the new rows pad to its width and R is within the kernel's."""
    N, d = shape
    if sorted_copy:
        return "the bank was built from unsorted labels and keeps a class-sorted copy, whose rows are not the caller's"
    if not (split or packed):
        return "a norms-only bank holds no prepared rows to refresh (build a new ops.SplitBank)"
    if width + pad != d:
        return f"new rows of width {width} do not pad to the bank's width {d}"
    if R > BANK_UPDATE_MAX_ROWS:
        return f"{R} rows in one call are above {BANK_UPDATE_MAX_ROWS}"
    return None


def _bank_node_save(ctx, qc, lse, out, ls, window, exclude, kind_id, operands, bank, logw, logw_src, values=None):
    """What the autograd nodes of the heads over a resident bank keep for their backward.  Saved tensors: the queries, lse,
    out, a clip scale and the window -- nothing of size B x N.  Beside them the constants the backward recomputes the scores
    from, each with what tells a write: the bank's ``operands`` and its ``writes`` count (SplitBank.update_rows writes them
    in place), the weights as the kernels read them with the caller's tensor and its version (an in-place write bumps it),
    the value head's BankValues."""
    ctx.save_for_backward(qc, lse, out, *([ls] if ls is not None else []), *(window if window is not None else []))
    ctx.bank = operands
    ctx.bank_writes = (bank, bank.writes)
    ctx.logw = None if logw is None else (logw, logw_src, logw_src._version)
    ctx.values = values
    ctx.meta = (kind_id, ls is not None, window is not None, exclude)


def _bank_node_load(ctx, entry):
    """-> (q, lse, out, clip scale or None, lo, hi, weights or None, kind_id, exclude) as _bank_node_save recorded them, after
    the refusal of a constant written since the forward (RuntimeError; ``entry``: the public name in front)."""
    kind_id, has_ls, windowed, exclude = ctx.meta
    saved = list(ctx.saved_tensors)
    qc, lse, out = saved[:3]
    ls = saved[3] if has_ls else None
    lo, hi = saved[-2:] if windowed else (None, None)
    if ctx.bank_writes[0].writes != ctx.bank_writes[1]:
        raise RuntimeError(f"{entry}: the bank was written (SplitBank.update_rows) between this forward and its "
                           "backward, which recomputes the scores from the bank: call backward() first, then update")
    if ctx.logw is not None and ctx.logw[1]._version != ctx.logw[2]:
        raise RuntimeError(f"{entry}: row_logw was written in place between this forward and its backward, which "
                           "recomputes the weighted scores from it: call backward() first, then change the weights")
    if ctx.values is not None and ctx.values.stale():
        raise RuntimeError(f"{entry}: the tensor the BankValues was prepared from was written between this forward "
                           "and its backward (the prepared rows no longer stand for it): build a new ops.BankValues")
    return qc, lse, out, ls, lo, hi, ctx.logw and ctx.logw[0], kind_id, exclude


class _NWHeadBankFn(torch.autograd.Function):
    """autograd node of nw_head_bank: today's inference call forward.  Backward: ONE query / weights call when q, the clip
    scale or row_logw needs it -- nw_bwd_query_f32, with support weights nw_bwd_query_weighted_f32, or nw_bwd_query_logw_f32
    when the weights need a gradient too (it goes to the last input, the caller's tensor; without gq when only they learn) --
    and, with ``support_grad``, nw_bwd_bank_support_f32 for the bank rows `s`, the third input.  Nothing of size B x N."""

    @staticmethod
    def forward(ctx, q, logit_scale, s, call, n_classes, kind_id, window, exclude, bank, logw=None, logw_src=None):
        """``s``: the bank rows when their gradient is wanted, else None; ``call``: the _Call nw_head_bank resolved (``q`` is
        its queries, an argument of its own for autograd); ``window``: None or (lo, hi) int32; ``bank``: the SplitBank the
        call reads; ``logw``: None or the (N,) fp32 support weights as the kernels read them (_row_logw), ``logw_src`` the
        caller's tensor they came from (the same one, or what a conversion copied)."""
        _, sc, syc, sn2, ssplit, sscale, opts = call
        lib = _lib.load()
        qc = _f32c(q)
        B, d = qc.shape
        N, dev = ssplit.shape[0], qc.device
        out = torch.empty(B, n_classes, dtype=torch.float32, device=dev)
        lse = torch.empty(B, dtype=torch.float32, device=dev)
        ls = None if logit_scale is None else _f32c(logit_scale)
        lo, hi = window if window is not None else (None, None)
        if logw is None and window is None:
            st = _stream(qc)
            ws, ws_bytes = _fwd_workspace(lib, B, N, d, n_classes, dev, st)
            with _OnDevice(dev):
                _lib.check(lib.nw_fwd_f32(_ptr(qc), _ptr(sc), _ptr(syc), _ptr(sn2), _ptr(ssplit), _ptr(sscale), _ptr(out), None,
                                          _ptr(lse), None, _ptr(ws), ws_bytes, B, N, d, n_classes, kind_id, _ptr(ls), 0, 0, opts,
                                          st), "nw_fwd_f32")
        else:
            _bank_head_fwd(qc, call, syc, logw, lo, hi, exclude, out, lse, kind_id, ls)
        _bank_node_save(ctx, qc, lse, out, ls, window, exclude, kind_id, (ssplit, sscale, sn2, syc), bank, logw, logw_src)
        # the fp32 rows the bank's forms were prepared from, at the bank's width (read for the 2 r s term), and what `s` is
        ctx.s_rows = None if s is None else (bank.rows if bank.rows is not None else _f32c(s), s.shape[1], s.dtype)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout):
        qc, lse, out, ls, lo, hi, logw, kind_id, exclude = _bank_node_load(ctx, "nw_head_bank")
        g = _f32c(gout)
        want_glogw = logw is not None and ctx.needs_input_grad[10]
        need_q = ctx.needs_input_grad[0] or (ls is not None and ctx.needs_input_grad[1])
        gq = gls = ga = gs = None
        if want_glogw or need_q:      # without gq (no second pass over the bank) when only the weights (and the rows) learn
            gq, gls, ga = _bank_head_bwd(qc, ctx.bank, logw, lo, hi, exclude, lse, out, g, kind_id, ls,
                                         not want_glogw or need_q, want_glogw)
        if ctx.s_rows is not None and ctx.needs_input_grad[2]:
            s_rows, width, dtype = ctx.s_rows
            gs = _bank_support_bwd(qc, s_rows, ctx.bank, logw, lo, hi, exclude, lse, out, g, kind_id, ls)
            if width != gs.shape[1]:
                gs = gs[:, :width]
            gs = gs.to(dtype)
        return (gq if ctx.needs_input_grad[0] else None, gls if ls is not None and ctx.needs_input_grad[1] else None, gs, None,
                None, None, None, None, None, None, ga if ga is None else ga.to(ctx.logw[1].dtype))


def _bank_support_bwd(q, s_rows, operands, logw, lo, hi, exclude, lse, out, gout, kind_id, ls, query_chunks=0):
    """The one call of the gradient of the head over a resident bank w.r.t. the bank rows (nw_bwd_bank_support_f32) -> gs (N, d)
    fp32.  ``s_rows``: the fp32 rows the bank's forms were prepared from, at the bank's width; the rest as _bank_head_bwd."""
    lib = _lib.load()
    ssplit, sscale, sn2, syc = operands
    (B, d), N, C, dev = q.shape, ssplit.shape[0], out.shape[1], q.device
    gs = torch.empty(N, d, dtype=torch.float32, device=dev)
    ws_bytes = lib.nw_bwd_bank_support_workspace_bytes(B, N, d, C, int(query_chunks))
    ws = _workspace(ws_bytes, dev)
    with _OnDevice(dev):
        _lib.check(lib.nw_bwd_bank_support_f32(_ptr(q), _ptr(s_rows), _ptr(ssplit), _ptr(sscale), _ptr(sn2), _ptr(syc), _ptr(logw),
                                               _ptr(lo), _ptr(hi), int(exclude), _ptr(lse), _ptr(out), _ptr(gout), _ptr(gs),
                                               _ptr(ws), ws_bytes, B, N, d, C, kind_id, _ptr(ls), int(query_chunks), _stream(q)),
                   "nw_bwd_bank_support_f32")
    return gs


def nw_head_bank(q, s, sy, n_classes, bank, kind="euclidean", logit_scale=None, row_window=None, exclude=False, row_logw=None,
                 support_grad=False):
    """The head over a RESIDENT bank, differentiable in the queries (and a clip ``logit_scale``) with the bank a constant
    -> (B,C) log-probabilities.  For fine-tuning a featurizer against a frozen or periodically refreshed bank, a
    leave-one-out training loss (``row_window`` / ``exclude`` as in nw_head_window), input gradients of 'full' inference,
    test-time adaptation.  `s` must not require grad: ``nw_head`` is the call for support gradients.

    Forward: the inference call as it is -- nw_fwd_f32 over the bank with its log-sum-exp, or nw_fwd_window_f32 -- so the
    output equals ``nw_head(..., support_cache=bank[, row_window=...])`` under no_grad bit for bit.  Backward:
    nw_bwd_query_f32, which recomputes the scores tile by tile on the split-fp16 matrix cores and contracts them with the
    bank rows in the same kernel: no (B,N) buffer is saved or filled (nw_head's route keeps three) and no support gradient
    is computed.  Route (head_bank_route): that kernel whenever the bank holds split rows without a class-sorted copy and
    the queries pad to its width; otherwise (an fp16 or norms-only bank, unsorted labels, N <= 25, a width that is no
    multiple of 32 after padding) nw_head's route without a window, NWHipError with one.

    row_logw: SUPPORT WEIGHTS as in nw_head_window.  A tensor that does not require grad is a constant like the bank;
    writing it in place between forward and backward is refused like a bank update, either way.  Forward
    nw_fwd_weighted_f32, backward nw_bwd_query_weighted_f32, wherever the rule above gives the kernel
    (head_weighted_route); where it does not, the gradient is refused with or without a window (NWHipError: nw_head's
    matrix route does not know the weights).
    LEARNABLE weights: when ``row_logw.requires_grad`` -- a leaf or any graph tensor, ``beta[labels]``, ``param + mask`` --
    the gradient flows to it as well, in its dtype: ga_j = sum_b W_bj (dP_b[y_j] - t_b), the column sums of what the query
    gradient contracts with the bank rows, from the same kernel (nw_bwd_query_logw_f32, DESIGN 4.8i: no (B, N) matrix; a
    row at -inf and a row no query admits get exactly 0).  One backward entry per case: that one when the weights need a
    gradient -- without gq, i.e. without the second pass over the bank rows, when neither `q` nor a clip scale does --
    and the entries above, unchanged, otherwise.  Where the kernel does not serve (the cases above) the gradient to the
    weights is refused (NWHipError); without a window nw_scores + a + nw_aggregate is the way through the score matrix.

    support_grad: LEARNABLE BANK ROWS (prototypes, a condensed support set, a bank trained end to end).  With
    ``support_grad=True`` and ``s.requires_grad`` the gradient flows to `s` as well, in its dtype (on a padded bank: the
    caller's columns): gs_j = sum_b A_bj q_b + 2 (sum_b r_bj) s_j from nw_bwd_bank_support_f32, which recomputes
    the coefficients of the query gradient tile by tile and contracts them with the queries: no (B, N) matrix; a row at -inf
    and a row no query admits get exactly 0.  The forward and the gradients to q, the clip scale and row_logw are those of
    the call without the keyword, bit for bit, and when only the rows learn no query-gradient call is made.  The bank must
    be brought up to date after the optimizer wrote `s` (``SplitBank.refresh``).  Route (head_bank_support_route): that
    kernel wherever the rule above gives the kernels; else nw_head's matrix route without a window and weights, NWHipError
    with either.  Without the keyword, or with an `s` that does not require grad, nothing changes."""
    if not isinstance(bank, SplitBank):
        raise TypeError("nw_head_bank runs over a prepared bank: pass ops.SplitBank(support)")
    grad = torch.is_grad_enabled()
    grad_s = bool(support_grad and grad and s.requires_grad)
    if grad and s.requires_grad and not grad_s:
        raise ValueError("nw_head_bank: the bank is a constant here and `s` requires grad; nw_head(q, s, sy, ..., "
                         "support_cache=bank) is the call for support gradients")
    _need_hip(q, s, sy, logit_scale)
    if s.dim() != 2 or sy.dim() != 1 or sy.shape[0] != s.shape[0] or not bank.matches(s):
        raise ValueError("nw_head_bank: `s` (N,d) must be the tensor the bank was prepared from and `sy` its (N,) labels")
    kid = _kind_id(kind)
    if kid == SCORE_KINDS["clip"] and logit_scale is None:
        raise ValueError("clip kernel needs logit_scale")
    grad_logw = grad and torch.is_tensor(row_logw) and row_logw.requires_grad
    if not (grad_s or (grad and (q.requires_grad or (logit_scale is not None and logit_scale.requires_grad) or grad_logw))):
        return nw_head(q, s, sy, n_classes, kind, logit_scale, support_cache=bank, row_window=row_window, exclude=exclude,
                       row_logw=row_logw)
    C = int(n_classes)
    _check_label_range(None, bank.label_max, C)
    logw = None if row_logw is None else _row_logw(row_logw, s.shape[0], q.device, "nw_head_bank")
    facts = dict(split=bank.split is not None, sorted_copy=bank.sorted_rows is not None, shape=bank.shape, pad=bank.pad,
                 width=q.shape[1], B=q.shape[0], n_classes=C)
    why = None if grad_s else head_bank_refusal(**facts)
    if grad_s and head_bank_support_route(window=row_window is not None, weights=logw is not None, **facts) == "matrix":
        return nw_head(q, s, sy, C, kind, logit_scale, support_cache=bank)
    if why is not None:
        if grad_logw:
            raise NWHipError(f"nw_head_bank(row_logw=...) has no route for the gradient to the weights here: {why}.  Without "
                             "a window the composition ops.nw_aggregate(ops.nw_scores(q, s, support_cache=bank) + a, sy, C) "
                             "(nw_scores + a + nw_aggregate) differentiates in a through the (B, N) score matrix")
        if logw is not None:
            raise NWHipError(f"nw_head_bank(row_logw=...) has no gradient route here: {why}")
        if row_window is None:
            return nw_head(q, s, sy, C, kind, logit_scale, support_cache=bank)
        raise NWHipError(f"nw_head_bank(row_window=...) has no gradient route here: {why}")
    if row_window is None and logw is None:
        # nw_head's inference call over the bank (the rows are the bank's: a learnable `s` is not handed to the graph here)
        call = _resolve(bank, q, s.detach() if grad_s else s, sy, C, False, False, False, 0, None, False)
        window = None
    else:
        call = _resolve_scores(bank, q)._replace(sy=_i64c(sy))
        window = None if row_window is None else tuple(_row_window(row_window, q.shape[0], q.device))
    return _NWHeadBankFn.apply(call.q, logit_scale, s if grad_s else None, call, C, kid, window, bool(exclude), bank, logw,
                               row_logw)


def head_values_grad_route(*, split, sorted_copy, shape, pad, width, B, T):
    """Which route serves the gradients of ``nw_head_values_bank``, beside head_values_route and over the same plain facts:
    "fused" (the value head's two launches forward, nw_bwd_values_query_f32 backward: no (B, N) buffer) exactly where
    head_values_route says "fused"; else "matrix": the differentiable composition nw_scores over the bank, + row_logw, the
    window's mask, torch.softmax and a matmul with the values -- windows and weights included, so no shape is refused."""
    return head_values_route(split=split, sorted_copy=sorted_copy, shape=shape, pad=pad, width=width, B=B, T=T)


def _scores_support_grad(q, s, sc, g, kind_id, scale=None):
    """Gradient of the (B, N) score matrix ``sc`` = scores(q, s) w.r.t. the SUPPORT rows `s` under the upstream gradient `g`
    -> (N, d): the transposes of _ScoresFn.backward's closed forms for the queries (bwd_coeff.h), in plain torch ops on
    whatever device and float dtype the arguments have.  The same conventions: no gradient passes at a distance of exactly 0
    (the euclidean kinds), and a row F.normalize's clamp holds (|s_j| <= 1e-12) gets no share through its norm.  ``scale``:
    exp(logit_scale), clip alone."""
    if kind_id == SCORE_KINDS["dotproduct"]:
        return g.t() @ q
    if kind_id == SCORE_KINDS["euclidean"]:
        a = torch.where(sc == 0, torch.zeros_like(g), g / -sc)
        return a.t() @ q - a.sum(0)[:, None] * s
    nq, ns = q.norm(dim=1, keepdim=True).clamp_min(1e-12), s.norm(dim=1, keepdim=True)
    nsc = ns.clamp_min(1e-12)
    if kind_id == SCORE_KINDS["hypersphere_euclidean"]:
        gc, c = torch.where(sc == 0, torch.zeros_like(g), g / -sc), 1.0 - 0.5 * sc * sc
    elif kind_id == SCORE_KINDS["cosine"]:
        gc, c = g, sc
    else:
        gc, c = g * scale, sc / scale
    through_norm = torch.where(ns > 1e-12, (gc * c).sum(0)[:, None], torch.zeros_like(ns))   # (the clamp passes none)
    return (gc.t() @ (q / nq) - through_norm * (s / nsc)) / nsc


class _ScoresFn(torch.autograd.Function):
    """``nw_scores`` with a gradient to the queries, to a clip ``logit_scale`` and to the supports: the score matrix of the
    "matrix" route of nw_head_values_bank.  Forward: nw_scores, as it is.  Backward: the closed forms of bwd_coeff.h in
    torch ops over the saved (B, N) scores -- a = g df/ddot, gq = a @ s + 2 rq q -- two (B, N) x (N, d) products; the
    zero sub-gradient at distance 0 and F.normalize's clamp are those of the kernels.  The supports' gradient
    (_scores_support_grad: the transposes) is computed only when `s` needs it."""

    @staticmethod
    def forward(ctx, q, logit_scale, s, kind, bank):
        sc = nw_scores(q, s, kind, logit_scale, support_cache=bank)
        ctx.save_for_backward(q, s, sc, *([logit_scale] if logit_scale is not None else []))
        ctx.kind = _kind_id(kind)
        return sc

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        q, s, sc = ctx.saved_tensors[:3]
        sdtype = s.dtype
        q, s, kid, gls = q.float(), s.float(), ctx.kind, None
        scale = ctx.saved_tensors[3].float().exp() if kid == SCORE_KINDS["clip"] else None
        gs = _scores_support_grad(q, s, sc, g, kid, scale).to(sdtype) if ctx.needs_input_grad[2] else None
        if not (ctx.needs_input_grad[0] or (scale is not None and ctx.needs_input_grad[1])):
            return None, None, gs, None, None
        if kid == SCORE_KINDS["dotproduct"]:
            return g @ s, None, gs, None, None
        if kid == SCORE_KINDS["euclidean"]:
            a = torch.where(sc == 0, torch.zeros_like(g), g / -sc)
            return a @ s - a.sum(1, keepdim=True) * q, None, gs, None, None
        nq, ns = q.norm(dim=1, keepdim=True), s.norm(dim=1, keepdim=True).clamp_min(1e-12)
        nqc = nq.clamp_min(1e-12)
        if kid == SCORE_KINDS["hypersphere_euclidean"]:
            gc, c = torch.where(sc == 0, torch.zeros_like(g), g / -sc), 1.0 - 0.5 * sc * sc
        elif kid == SCORE_KINDS["cosine"]:
            gc, c = g, sc
        else:
            gc, c, gls = g * scale, sc / scale, (g * sc).sum().to(ctx.saved_tensors[3].dtype)
        through_norm = torch.where(nq > 1e-12, (gc * c).sum(1, keepdim=True), torch.zeros_like(nq))   # (the clamp passes none)
        return (gc @ (s / ns) - through_norm * (q / nqc)) / nqc, gls, gs, None, None


def _values_head_matrix(q, s, bank, vals, kind, logit_scale, logw, lo, hi, exclude):
    """The differentiable "matrix" composition of the value head -> (B, T): nw_scores over the bank (_ScoresFn), + ``logw``,
    the window's mask, torch.softmax, @ ``vals`` ((N, T) fp32), a dead query 0 in every column.  Autograd keeps the (B, N)
    matrices."""
    N = s.shape[0]
    x = _ScoresFn.apply(q, logit_scale, s, kind, bank)
    if logw is not None:
        x = x + logw
    if lo is not None:
        cols = torch.arange(N, device=q.device)
        keep = (cols >= lo[:, None]) & (cols < hi[:, None])
        x = x.masked_fill(keep if exclude else ~keep, float("-inf"))
    dead = ~(x > float("-inf")).any(dim=1, keepdim=True)       # (a softmax over nothing is NaN, and so is its gradient)
    return torch.softmax(x.masked_fill(dead, 0.0), dim=1).masked_fill(dead, 0.0) @ vals


def _values_query_bwd(qc, operands, values, logw, lo, hi, exclude, lse, out, gout, kind_id, ls):
    """ONE call of nw_bwd_values_query_f32 -> (gq, glogit_scale or None).  ``operands``: the bank's (split rows, scales,
    norms); ``values``: the BankValues; ``gout``: the upstream gradient, copied where it is not fp32, contiguous and 16-byte
    aligned."""
    lib = _lib.load()
    ssplit, sscale, sn2 = operands
    (B, d), N, Tp, dev = qc.shape, ssplit.shape[0], out.shape[1], qc.device
    g = _f32c(gout)
    if g.data_ptr() % 16:
        g = g.clone()
    gq = torch.empty_like(qc)
    gls = torch.empty((), dtype=torch.float32, device=dev) if ls is not None else None
    ws_bytes = lib.nw_bwd_values_query_workspace_bytes(B, N, d, Tp, 0)
    ws = _workspace(ws_bytes, dev)
    with _OnDevice(dev):
        _lib.check(lib.nw_bwd_values_query_f32(_ptr(qc), _ptr(ssplit), _ptr(sscale), _ptr(sn2), _ptr(values.split),
                                               _ptr(values.scale), _ptr(logw), _ptr(lo), _ptr(hi), int(bool(exclude)),
                                               _ptr(lse), _ptr(out), _ptr(g), _ptr(gq), _ptr(gls), _ptr(ws), ws_bytes, B, N, d,
                                               Tp, kind_id, _ptr(ls), 0, _stream(qc)), "nw_bwd_values_query_f32")
    return gq, gls


def _values_support_bwd(qc, operands, values, logw, lo, hi, exclude, lse, out, g, kind_id, ls, want_gvalues, want_glogw,
                        query_chunks=0):
    """ONE call of nw_bwd_values_support_f32 -> (gvalues (N, values.width) or None, glogw (N,) or None).  ``operands``: the
    bank's (split rows, scales, norms); ``g``: the fp32 upstream gradient, 16-byte aligned.  Without ``want_gvalues`` nothing
    of size N x T is allocated."""
    lib = _lib.load()
    ssplit, sscale, sn2 = operands
    (B, d), N, Tp, dev = qc.shape, ssplit.shape[0], out.shape[1], qc.device
    gv = torch.empty(N, Tp, dtype=torch.float32, device=dev) if want_gvalues else None
    ga = torch.empty(N, dtype=torch.float32, device=dev) if want_glogw else None
    ws_bytes = lib.nw_bwd_values_support_workspace_bytes(B, N, d, Tp, query_chunks, int(want_gvalues))
    ws = _workspace(ws_bytes, dev)
    with _OnDevice(dev):
        _lib.check(lib.nw_bwd_values_support_f32(_ptr(qc), _ptr(ssplit), _ptr(sscale), _ptr(sn2),
                                                 _ptr(values.rows) if want_glogw else None, _ptr(logw), _ptr(lo), _ptr(hi),
                                                 int(bool(exclude)), _ptr(lse), _ptr(out), _ptr(g), _ptr(gv), _ptr(ga), _ptr(ws),
                                                 ws_bytes, B, N, d, Tp, kind_id, _ptr(ls), query_chunks, _stream(qc)),
                   "nw_bwd_values_support_f32")
    return gv, ga


def _values_bank_support_bwd(qc, s_rows, operands, values, logw, lo, hi, exclude, lse, out, g, kind_id, ls, query_chunks=0):
    """ONE call of nw_bwd_values_bank_support_f32 -> gs (N, d) fp32, the value head's gradient w.r.t. the bank rows.
    ``s_rows``: the fp32 rows the bank's forms were prepared from, at the bank's width (read for the 2 r s term); the rest
    as _values_query_bwd."""
    lib = _lib.load()
    ssplit, sscale, sn2 = operands
    (B, d), N, Tp, dev = qc.shape, ssplit.shape[0], out.shape[1], qc.device
    gs = torch.empty(N, d, dtype=torch.float32, device=dev)
    ws_bytes = lib.nw_bwd_values_bank_support_workspace_bytes(B, N, d, Tp, int(query_chunks))
    ws = _workspace(ws_bytes, dev)
    with _OnDevice(dev):
        _lib.check(lib.nw_bwd_values_bank_support_f32(_ptr(qc), _ptr(s_rows), _ptr(ssplit), _ptr(sscale), _ptr(sn2),
                                                      _ptr(values.split), _ptr(values.scale), _ptr(logw), _ptr(lo), _ptr(hi),
                                                      int(bool(exclude)), _ptr(lse), _ptr(out), _ptr(g), _ptr(gs), _ptr(ws),
                                                      ws_bytes, B, N, d, Tp, kind_id, _ptr(ls), int(query_chunks), _stream(qc)),
                   "nw_bwd_values_bank_support_f32")
    return gs


class _NWValuesBankFn(torch.autograd.Function):
    """autograd node of nw_head_values_bank on the fused route: the inference launches forward (_values_head_fwd: the lse pass,
    nw_fwd_values_f32).  Backward: ONE call of nw_bwd_values_query_f32 when the queries or a clip scale need it and, with
    ``support_grad``, ONE call of nw_bwd_values_support_f32 for the values' source tensor (3rd input) and the caller's row_logw
    (11th input), each in its dtype; when only the weights learn nothing of size N x T is allocated.  With the bank rows `s`
    as the last input, ONE call of nw_bwd_values_bank_support_f32 for them; when only the rows learn, no other call.  Returns
    the padded (B, values.width) raw output; the slice to T and the logarithm are torch ops behind it.  Nothing of size
    B x N is saved."""

    @staticmethod
    def forward(ctx, q, logit_scale, vsrc, call, bank, values, kind_id, window, exclude, logw=None, logw_src=None, s=None):
        """``vsrc``: the tensor the values were prepared from when its gradient is wanted, else None; ``call``:
        _resolve_scores' _Call (``q`` is its queries, an argument of its own for autograd); ``values``: the BankValues;
        ``window``: None or (lo, hi) int32; ``logw`` / ``logw_src``: as in _NWHeadBankFn; ``s``: the bank rows when their
        gradient is wanted, else None."""
        qc = _f32c(q)
        if qc.data_ptr() % 16:
            qc = qc.clone()
        ls = None if logit_scale is None else _f32c(logit_scale)
        lo, hi = window if window is not None else (None, None)
        out, lse = _values_head_fwd(call._replace(q=qc), bank, values, logw, lo, hi, exclude, kind_id, ls)
        _bank_node_save(ctx, qc, lse, out, ls, window, exclude, kind_id, (call.operand, call.scale, call.norm2), bank, logw,
                        logw_src, values)
        ctx.vsrc = None if vsrc is None else (vsrc.dtype, tuple(vsrc.shape))
        # the fp32 rows the bank's forms were prepared from, at the bank's width (read for the 2 r s term), and what `s` is
        ctx.s_rows = None if s is None else (bank.rows if bank.rows is not None else _f32c(s), s.shape[1], s.dtype)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout):
        qc, lse, out, ls, lo, hi, logw, kind_id, exclude = _bank_node_load(ctx, "nw_head_values_bank")
        g = _f32c(gout)
        if g.data_ptr() % 16:
            g = g.clone()
        gq = gls = gv = ga = None
        if ctx.needs_input_grad[0] or (ls is not None and ctx.needs_input_grad[1]):
            gq, gls = _values_query_bwd(qc, ctx.bank, ctx.values, logw, lo, hi, exclude, lse, out, g, kind_id, ls)
        want_gv = ctx.vsrc is not None and ctx.needs_input_grad[2]
        want_ga = logw is not None and ctx.needs_input_grad[10]
        if want_gv or want_ga:
            gv, ga = _values_support_bwd(qc, ctx.bank, ctx.values, logw, lo, hi, exclude, lse, out, g, kind_id, ls, want_gv, want_ga)
        if gv is not None:
            T, Tp = ctx.vsrc[1][1], out.shape[1]
            gv = (gv if T == Tp else gv[:, :T]).to(ctx.vsrc[0])
        if ga is not None:
            ga = ga.to(ctx.logw[1].dtype)
        gs = None
        if ctx.s_rows is not None and ctx.needs_input_grad[11]:
            s_rows, width, dtype = ctx.s_rows
            gs = _values_bank_support_bwd(qc, s_rows, ctx.bank, ctx.values, logw, lo, hi, exclude, lse, out, g, kind_id, ls)
            if width != gs.shape[1]:
                gs = gs[:, :width]
            gs = gs.to(dtype)
        return gq, gls, gv, None, None, None, None, None, None, None, ga, gs


def nw_head_values_bank(q, s, bank, values, kind="euclidean", logit_scale=None, row_window=None, exclude=False, row_logw=None,
                        log=False, support_grad=False):
    """The VALUE head over a RESIDENT bank at training time: ``nw_head_values``, differentiable in the queries (and a clip
    ``logit_scale``) with the bank, the values and the weights constants -> (B, T) fp32.  For fine-tuning a featurizer against
    a frozen or periodically refreshed bank with regression targets, soft / mixup / distilled labels (``log=True`` and a KL or
    cross-entropy loss), embeddings to retrieve, or a leave-one-out regression loss over the bank's own rows (``row_window`` /
    ``exclude``).  The counterpart of nw_head_bank; arguments as in nw_head_values.

    With nothing requiring grad, or grad mode off, this IS nw_head_values(...): the same call, the same bits.  Otherwise, on
    the fused route, the forward is the inference launches as they are (the lse pass, nw_fwd_values_f32: bit-equal to
    nw_head_values under no_grad) and the backward ONE call of nw_bwd_values_query_f32, which recomputes the scores and
    c = gout @ values^T tile by tile on the split-fp16 matrix cores and contracts dS = W (c - gout . out) with the bank rows
    in the same kernel: the node saves q, lse, out and the window, nothing of size B x N.  The slice to T
    columns and ``log`` (log(out + 1e-12)) are torch ops behind the node.
    Route (head_values_grad_route): that kernel exactly where nw_head_values is fused; else (an fp16 or norms-only bank, a
    class-sorted copy, N <= 25, widths that do not pad, T > 16384) "matrix": nw_scores over the bank, + row_logw, the
    window's mask, torch.softmax and a matmul, through torch autograd and three (B, N) matrices -- no shape is refused.

    Constants: `s` must not require grad (ValueError; ``support_grad=True`` below lifts it); ``values`` or ``row_logw``
    that requires grad raises NWHipError (no
    gradient to either is computed here: the composition nw_scores + softmax + matmul differentiates in them through the
    (B, N) matrix).  On the fused route a bank written (SplitBank.update_rows), a ``row_logw`` written in place, or a
    BankValues gone stale between forward and backward is refused at backward (RuntimeError).

    Accuracy: c - gout . out cancels.  The error of c is ~2.4e-7 sum_t |gout_t values_jt| whatever the spread of the values
    among the rows, so value columns with a large common offset lose that many bits of the gradient: CENTRE such columns
    (the forward is linear in the values: add the offset back to the output).  Every value must be finite, in every row.

    ``support_grad=True``: LEARNABLE values and support weights.  Gradients flow to whichever of ``values`` and
    ``row_logw`` requires grad instead of the refusal above; `q` and ``logit_scale`` may require grad too, or not.  ``values``:
    the raw (N, T) tensor, or a BankValues whose source tensor is alive -- the gradient goes to that tensor, in its dtype (the
    source gone: NWHipError; after an optimiser step call ``BankValues.refresh()``).  ``row_logw``: a leaf or any graph
    tensor, any float dtype, as in nw_head_bank.  Fused route: the same forward; backward nw_bwd_values_query_f32 when the
    queries or the clip scale need it (gq's bits are those of the call without ``support_grad``) and ONE call of
    nw_bwd_values_support_f32, gvalues_j = sum_b W_bj gout_b and glogw_j = gvalues_j . values_j - sum_b W_bj (gout_b . out_b):
    no (B, N) buffer; when only the weights learn, nothing of size N x T either.  Matrix route: the graph tensors go through
    the composition.  With nothing on the support side requiring grad the keyword changes nothing.

    LEARNABLE BANK ROWS: with ``support_grad=True`` and ``s.requires_grad`` -- `s` still the tensor the bank
    was prepared from -- the gradient flows to `s` as well, in its dtype (on a padded bank: the caller's columns): the keys
    of a key-value memory, prototypes with regression targets, a condensed support set with soft labels.  Fused route: ONE
    more call, nw_bwd_values_bank_support_f32, gs_j = sum_b A_bj q_b + 2 (sum_b r_bj) s_j with (A, r) the query gradient's
    per-pair coefficients of dS = W (c - gout . out), recomputed tile by tile and contracted with the queries: no (B, N)
    buffer, nothing of size N x T; a row at -inf and a row no query admits get exactly 0.  The forward and the gradients to
    q, the clip scale, the values and row_logw are those of the call without a learnable `s`, bit for bit; when only the
    rows learn no other backward call is made.  The accuracy note above holds for gs too.  After the optimizer wrote `s`
    the bank must be brought up to date (``SplitBank.refresh``); a refresh or update_rows between forward and backward is
    refused at backward (RuntimeError).  Matrix route: nw_scores differentiates in `s` too (the transposed closed forms),
    windows and weights included.  Without the keyword an `s` that requires grad is refused as before."""
    _need_hip(q, s, logit_scale)
    if not isinstance(bank, SplitBank):
        raise TypeError("nw_head_values_bank runs over a prepared bank: pass ops.SplitBank(support)")
    grad = torch.is_grad_enabled()
    grad_s = bool(support_grad and grad and s.requires_grad)
    if grad and s.requires_grad and not grad_s:
        raise ValueError("nw_head_values_bank: the bank is a constant here and `s` requires grad")
    raw = values if torch.is_tensor(values) else None
    grad_v = bool(grad and (raw.requires_grad if raw is not None else getattr(values, "requires_grad", False)))
    grad_a = bool(grad and torch.is_tensor(row_logw) and row_logw.requires_grad)
    if (grad_v or grad_a) and not support_grad:
        raise NWHipError("nw_head_values_bank differentiates in the queries and a clip scale alone and does not detach silently: "
                         "values or row_logw requires grad.  The composition nw_scores + softmax + matmul differentiates in them")
    if grad_v or grad_a:
        _need_hip(raw, row_logw if torch.is_tensor(row_logw) else None)
    elif not (grad_s or (grad and (q.requires_grad or (logit_scale is not None and logit_scale.requires_grad)))):
        return nw_head_values(q, s, bank, values, kind, logit_scale, row_window=row_window, exclude=exclude, row_logw=row_logw,
                              log=log)
    if s.dim() != 2 or not bank.matches(s):
        raise ValueError("nw_head_values_bank: `s` (N,d) must be the tensor the bank was prepared from")
    if raw is not None:
        vsrc, values = raw, BankValues(raw, bank)
    elif isinstance(values, BankValues):
        vsrc = values.source()
        if grad_v and vsrc is None:
            raise NWHipError("nw_head_values_bank(support_grad=True): the tensor this BankValues was prepared from is gone, so "
                             "there is nothing for the gradient to the values to go to; build a new ops.BankValues")
    else:
        raise TypeError("nw_head_values_bank: values is an ops.BankValues or an (N,T) float tensor")
    N, T = s.shape[0], values.T
    if values.rows.shape[0] != N or values.rows.device != q.device:
        raise ValueError(f"nw_head_values_bank: the values hold {values.rows.shape[0]} rows on {values.rows.device} for a bank of "
                         f"{N} rows and queries on {q.device}")
    if values.stale():
        raise ValueError("nw_head_values_bank: the tensor this BankValues was prepared from was written since; build a new "
                         "ops.BankValues" + (" (or BankValues.refresh())" if grad_v or grad_a else ""))
    if q.dtype != torch.float32:
        q = q.float()
    B = q.shape[0]
    window = None if row_window is None else tuple(_row_window(row_window, B, q.device))
    logw = None if row_logw is None else _row_logw(row_logw, N, q.device, "nw_head_values_bank")
    kid = _kind_id(kind)
    if kid == SCORE_KINDS["clip"] and logit_scale is None:
        raise ValueError("clip kernel needs logit_scale")
    route = head_values_grad_route(split=bank.split is not None, sorted_copy=bank.sorted_rows is not None, shape=bank.shape,
                                   pad=bank.pad, width=q.shape[1], B=B, T=T)
    if route == "fused":
        # (queries padded by a torch op: autograd slices gq back; the rows of the call are the bank's: a learnable `s` goes to
        # the node as an input of its own)
        call = _resolve_scores(bank, q, s.detach() if grad_s else s)
        out = _NWValuesBankFn.apply(call.q, logit_scale, vsrc if grad_v else None, call, bank, values, kid, window,
                                    bool(exclude), logw, row_logw, s if grad_s else None)
        if values.width != T:
            out = out[:, :T]
    else:
        # the matrix composition differentiates in the graph tensors themselves
        vals = vsrc.float() if grad_v else values.rows[:, :T]
        a = row_logw.float() if grad_a else logw
        if B == 0 or N == 0:     # nothing to compute: zeros, tied to whatever requires grad
            out = torch.zeros(B, T, dtype=torch.float32, device=q.device) + 0.0 * sum(
                t.sum() for t, on in ((q, q.requires_grad), (vals, grad_v), (a, grad_a), (s, grad_s)) if on)
        else:
            lo, hi = window if window is not None else (None, None)
            out = _values_head_matrix(q, s, bank, vals, kind, logit_scale, a, lo, hi, bool(exclude))
    return torch.log(out + 1e-12) if log else out


def nw_partials(q, s, sy, n_classes, kind="euclidean", logit_scale=None, support_cache=None):
    """This rank's (m, den, num) over its shard of the bank; no grad.  ``support_cache``: the
    shard's SplitBank (see there; an fp16 bank: the partials of the rounded features)."""
    _need_hip(q, s, sy, logit_scale)
    qc = _f32c(q)
    packed = torch.empty(qc.shape[0], n_classes + 2, dtype=torch.float32, device=qc.device)
    return nw_partials_into(packed, qc, _f32c(s), sy, n_classes, kind, logit_scale, cache=support_cache)


def nw_partials_into(packed, qc, sc, sy, n_classes, kind="euclidean", logit_scale=None, ws=None, sn2=None,
                     cache=None, persistent_wgs=0):
    """Write partials into ``packed`` laid out as [m (B) | den (B) | num (B*C)] (flat, contiguous):
    one buffer = one collective.  ``qc`` / ``sc`` must already be fp32 contiguous HIP tensors.  ``ws``: a scratch buffer
    of the caller's (used when large enough, see _fwd_workspace); ``cache``: the SplitBank of ``sc``."""
    _partials(packed, qc, sc, sy, n_classes, kind, logit_scale, ws, sn2, cache, persistent_wgs)
    return packed


def _partials(packed, qc, sc, sy, n_classes, kind, logit_scale, ws=None, sn2=None, cache=None, persistent_wgs=0, own_ws=False):
    """nw_partials_into; returns the scratch buffer it used (``own_ws``: ShardedBank keeps its own and lets it grow here)."""
    lib = _lib.load()
    call = _resolve(cache, qc, sc, sy, n_classes, half=True, persistent_wgs=persistent_wgs, norm2=sn2)
    qc, C = call.q, int(n_classes)
    (B, d), N = qc.shape, call.s.shape[0]
    st = _stream(qc)
    ws, ws_bytes = _fwd_workspace(lib, B, N, d, C, qc.device, st, ws, own_ws)
    flat = packed.view(-1)
    m, den, num = flat[:B], flat[B:2 * B], flat[2 * B:2 * B + B * C]
    ls = None if logit_scale is None else _f32c(logit_scale)
    with _OnDevice(qc.device):
        _lib.check(lib.nw_fwd_partial_f32(_ptr(qc), _ptr(call.s), _ptr(call.sy), _ptr(call.norm2), _ptr(call.operand),
                                          _ptr(call.scale), _ptr(m), _ptr(den), _ptr(num), _ptr(ws), ws_bytes, B, N, d, C,
                                          _kind_id(kind), _ptr(ls), call.opts, st), "nw_fwd_partial_f32")
    return ws


def nw_merge(packed_all, B, n_classes, out=None, class_lo=None, c_local=None):
    """packed_all: (G, L) all-gathered partial buffers, each row [m (B) | den (B) | num (B*CL)] -> (B,C)
    log-probs.  CL = n_classes, or ``c_local`` when every shard only carries the class window
    [class_lo[g], class_lo[g] + c_local).  The merge kernel reads the sections in place."""
    _need_hip(packed_all, class_lo)
    lib = _lib.load()
    assert packed_all.dim() == 2 and packed_all.is_contiguous() and packed_all.dtype == torch.float32
    G, L = packed_all.shape
    C = int(n_classes)
    CL = C if class_lo is None else int(c_local)
    assert L >= 2 * B + B * CL
    dev = packed_all.device
    if out is None:
        out = torch.empty(B, C, dtype=torch.float32, device=dev)
    base = packed_all.data_ptr()
    with _OnDevice(dev):
        _lib.check(lib.nw_merge_finalize_f32(base, base + 4 * B, base + 8 * B, _ptr(out), G, B, C, L, L, L,
                                             _ptr(class_lo), CL, _stream(packed_all)), "nw_merge_finalize_f32")
    return out


def scale_shift_relu(x, scale, shift, relu=True):
    """out = max(x * scale[c] + shift[c], 0) for an (n, c, h, w) fp32 activation whose (c, h, w) part is
    contiguous (a channel prefix of a wider slab is fine): eval-mode BatchNorm + ReLU in one pass."""
    _need_hip(x, scale, shift)
    n, c, h, w = x.shape
    hw = h * w
    if x.dtype != torch.float32 or (n * c * hw and (x.stride(3) != 1 or x.stride(2) != w or x.stride(1) != hw)):
        x = x.float().contiguous()
    out = torch.empty(n, c, h, w, dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().nw_scale_shift_relu_f32(_ptr(x), _ptr(_f32c(scale)), _ptr(_f32c(shift)), _ptr(out), n, c, hw,
                                                       x.stride(0) if n > 1 else c * hw, int(bool(relu)), _stream(x)),
                   "nw_scale_shift_relu_f32")
    return out


def bias_act_nhwc_(x, bias, residual=None, relu=True):
    """IN PLACE x <- act(x + bias[c] (+ residual)) for an (n, c, h, w) fp32 activation in channels_last memory format
    (c % 4 == 0): the folded BatchNorm bias, a ResNet block's identity and the ReLU behind a bias-free convolution in one
    pass.  Returns x."""
    _need_hip(x, bias, residual)
    n, c, h, w = x.shape
    ok = lambda t: t.dtype == torch.float32 and t.shape == x.shape and t.is_contiguous(memory_format=torch.channels_last)
    if not ok(x) or (residual is not None and not ok(residual)) or c % 4:
        raise ValueError("bias_act_nhwc_: fp32 channels_last (n, c, h, w) tensors with c % 4 == 0")
    with _OnDevice(x.device):
        _lib.check(_lib.load().nw_bias_act_nhwc_f32(_ptr(x), _ptr(_f32c(bias)), _ptr(residual), int(bool(relu)), _ptr(x),
                                                    n * h * w, c, _stream(x)), "nw_bias_act_nhwc_f32")
    return x


def scale_shift_relu_avgpool2(x, scale, shift, relu=True):
    """avg_pool2d(max(x * scale[c] + shift[c], 0), 2) in one pass: (n, c, h, w) -> (n, c, h // 2, w // 2)."""
    _need_hip(x, scale, shift)
    x, bstride = _plane_view(x)
    n, c, h, w = x.shape
    out = torch.empty(n, c, h // 2, w // 2, dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().nw_scale_shift_relu_avgpool2_f32(_ptr(x), _ptr(_f32c(scale)), _ptr(_f32c(shift)), _ptr(out), n, c, h, w,
                                                                bstride, int(bool(relu)), _stream(x)),
                   "nw_scale_shift_relu_avgpool2_f32")
    return out


def conv1x1(x, weight_t, bias=None, pre_scale=None, pre_shift=None, pre_relu=False, post_relu=False, cin=None):
    """out = post(bias + W . pre(x)) for an (n, c, h, w) fp32 activation whose (c, h, w) part is contiguous (a channel
    prefix of a wider slab is fine): pre = optional per-channel scale/shift (eval-mode BatchNorm) + ReLU, W given
    transposed as weight_t (cin rounded up to 16 with zero rows, cout), post = optional ReLU.  One matrix-core
    kernel (nw_conv1x1_f32)."""
    _need_hip(x, weight_t, bias, pre_scale, pre_shift)
    x, bstride = _plane_view(x)
    n, c, h, w = x.shape
    cin = c if cin is None else int(cin)
    cout = weight_t.shape[1]
    if c != cin or weight_t.shape[0] != (cin + 15) // 16 * 16 or not weight_t.is_contiguous():
        raise ValueError(f"conv1x1: input has {c} channels, weight_t must be ({(c + 15) // 16 * 16}, cout) contiguous")
    lib = _lib.load()
    out = torch.empty(n, cout, h, w, dtype=torch.float32, device=x.device)
    ws_bytes = lib.nw_conv1x1_workspace_bytes(n, cin, cout, h * w)
    ws = _workspace(ws_bytes, x.device) if ws_bytes else None
    with torch.cuda.device(x.device):
        _lib.check(lib.nw_conv1x1_f32(_ptr(x), bstride, _ptr(pre_scale), _ptr(pre_shift), int(bool(pre_relu)),
                                      _ptr(weight_t), _ptr(bias), int(bool(post_relu)), _ptr(out), cout * h * w,
                                      _ptr(ws), ws_bytes, n, cin, cout, h * w, _stream(x)), "nw_conv1x1_f32")
    return out


def conv3x3_weight(w):
    """(cout, cin, 3, 3) -> the operand of conv3x3: (ceil(cin / 8), 9, 8, cout), channels past cin zero."""
    cout, cin = w.shape[:2]
    pad = (-cin) % 8
    if pad:
        w = torch.cat((w, w.new_zeros(cout, pad, 3, 3)), 1)
    return w.reshape(cout, (cin + pad) // 8, 8, 9).permute(1, 3, 2, 0).contiguous()


def conv3x3(x, weight_t, cin, bias=None, residual=None, post_relu=False, out=None):
    """3x3 convolution, stride 1, padding 1, of an (n, c, h, w) fp32 activation whose (c, h, w) part is contiguous (a
    channel prefix of a slab is fine), weight_t from conv3x3_weight; bias / residual / ReLU behind it in the same
    kernel; `out`: an (n, cout, h, w) view with contiguous (cout, h, w) part to write into (a channel window of a slab)."""
    _need_hip(x, weight_t, bias, residual, out)
    x, bstride = _plane_view(x)
    n, c, h, w = x.shape
    cout = weight_t.shape[3]
    if c != cin or tuple(weight_t.shape[:3]) != ((cin + 7) // 8, 9, 8) or not weight_t.is_contiguous():
        raise ValueError("conv3x3: weight_t must be conv3x3_weight(w) of a (cout, cin, 3, 3) weight with cin = x's channels")
    if out is None:
        out = torch.empty(n, cout, h, w, dtype=torch.float32, device=x.device)
    elif out.shape != (n, cout, h, w) or out.dtype != torch.float32 or (out.numel() and (
            out.stride(3) != 1 or out.stride(2) != w or out.stride(1) != h * w)):
        raise ValueError("conv3x3: `out` must be (n, cout, h, w) fp32 with a contiguous (cout, h, w) part")
    obs = out.stride(0) if n > 1 else cout * h * w
    rbs = 0
    if residual is not None:
        residual, rbs = _plane_view(residual)
        if residual.shape != (n, cout, h, w):
            raise ValueError("conv3x3: residual must have the output's shape")
    lib = _lib.load()
    ws_bytes = lib.nw_conv3x3_workspace_bytes(n, cin, cout, h, w)   # partial tiles when K is split over workgroups (7x7 planes)
    ws = _workspace(ws_bytes, x.device) if ws_bytes else None
    with _OnDevice(x.device):
        _lib.check(lib.nw_conv3x3_f32(_ptr(x), bstride, _ptr(weight_t), _ptr(bias), _ptr(residual), rbs, int(bool(post_relu)),
                                      _ptr(out), obs, _ptr(ws), ws_bytes, n, cin, cout, h, w, _stream(x)), "nw_conv3x3_f32")
    return out


def pad_rows16(w_t):
    """(cin, cout) -> (cin rounded up to 16, cout) with zero rows: the weight operand of conv1x1."""
    cin = w_t.shape[0]
    pad = (-cin) % 16
    return w_t.contiguous() if pad == 0 else torch.cat((w_t, w_t.new_zeros(pad, w_t.shape[1]))).contiguous()


def _plane_view(x):
    """(n, c, h, w) fp32 with a contiguous (c, h, w) part (batch stride free) -> (tensor, batch stride)."""
    n, c, h, w = x.shape
    if x.dtype != torch.float32 or (x.numel() and (x.stride(3) != 1 or x.stride(2) != w or x.stride(1) != h * w)):
        x = x.float().contiguous()
    return x, (x.stride(0) if n > 1 else c * h * w)


class _BNReLUTrainFn(torch.autograd.Function):
    """relu(batch_norm(x) [+ residual]) in training mode: nw_bn_relu_train_fwd_f32 / _bwd_f32 (one kernel each)."""

    @staticmethod
    def forward(ctx, x, weight, bias, residual, bn, relu, passthrough=False):
        lib = _lib.load()
        xv, bstride = _plane_view(x.detach())
        n, c, h, w = xv.shape
        rv = None
        if residual is not None:
            rv = residual.detach()
            if rv.shape != xv.shape:
                raise ValueError("residual must have the shape of x")
            rv = rv if (rv.dtype == torch.float32 and rv.is_contiguous()) else rv.float().contiguous()
        y = torch.empty(n, c, h, w, dtype=torch.float32, device=xv.device)
        mean = torch.empty(c, dtype=torch.float32, device=xv.device)
        invstd = torch.empty_like(mean)
        track = bn.track_running_stats and bn.running_mean is not None
        momentum, nbt = 0.0, None
        if track:
            if bn.momentum is None:                 # cumulative moving average: the factor needs the count on the host
                bn.num_batches_tracked += 1
                momentum = 1.0 / float(bn.num_batches_tracked)
            else:
                momentum, nbt = float(bn.momentum), bn.num_batches_tracked   # counted inside the kernel
        wc, bc = _f32c(weight), _f32c(bias)
        with torch.cuda.device(xv.device):
            _lib.check(lib.nw_bn_relu_train_fwd_f32(_ptr(xv), _ptr(rv), _ptr(wc), _ptr(bc),
                                                    _ptr(bn.running_mean) if track else None,
                                                    _ptr(bn.running_var) if track else None, _ptr(y), _ptr(mean),
                                                    _ptr(invstd), _ptr(nbt), n, c, h * w, bstride, momentum, float(bn.eps),
                                                    int(relu), _stream(xv)), "nw_bn_relu_train_fwd_f32")
        ctx.save_for_backward(xv, wc, bc, mean, invstd, *(() if rv is None else (rv,)))
        ctx.relu, ctx.bstride, ctx.passthrough = relu, bstride, passthrough
        if passthrough:                 # (y, x): x leaves again so that it has ONE consumer; its other gradient
            ctx.set_materialize_grads(False)   # arrives in backward and is added inside the kernel
            return y, x.view_as(x)
        return y

    @staticmethod
    def backward(ctx, gy, gpass=None):
        lib = _lib.load()
        xv, wc, bc, mean, invstd, *rest = ctx.saved_tensors
        rv = rest[0] if rest else None
        n, c, h, w = xv.shape
        if gy is None:                  # only the pass-through output was used
            return gpass, None, None, None, None, None, None
        gy = _f32c(gy)
        acc, acc_bs = None, 0
        if gpass is not None:
            acc, acc_bs = _plane_view(gpass)
        dx = torch.empty(n, c, h, w, dtype=torch.float32, device=xv.device)
        dr = torch.empty_like(dx) if rv is not None else None
        dg, db = torch.empty_like(mean), torch.empty_like(mean)
        with torch.cuda.device(xv.device):
            _lib.check(lib.nw_bn_relu_train_bwd_f32(_ptr(xv), _ptr(rv), _ptr(gy), _ptr(wc), _ptr(bc), _ptr(mean),
                                                    _ptr(invstd), _ptr(dx), _ptr(dr), _ptr(dg), _ptr(db), _ptr(acc), acc_bs,
                                                    n, c, h * w, ctx.bstride, int(ctx.relu), _stream(xv)),
                       "nw_bn_relu_train_bwd_f32")
        return dx, dg, db, dr, None, None, None


def bn_relu_train(x, bn, relu=True, residual=None, passthrough=False):
    """relu(bn(x)) -- or relu(bn(x) + residual), the tail of a ResNet block -- for a BatchNorm2d in training mode
    (batch statistics, running statistics updated), fp32 NCHW on the MI355X.
    passthrough=True returns (y, x'): x' is x again, to be used by x's OTHER consumer, so that the gradient
    coming back through it is added to dx inside the backward kernel."""
    _need_hip(x, bn.weight, bn.bias, residual)
    if not (bn.affine and bn.weight is not None):
        raise ValueError("bn_relu_train needs an affine BatchNorm2d")
    if x.shape[0] * x.shape[2] * x.shape[3] <= 1:      # torch.nn.functional.batch_norm's own check
        raise ValueError(f"Expected more than 1 value per channel when training, got input size {tuple(x.shape)}")
    if bn.running_mean is not None and (bn.running_mean.dtype != torch.float32 or not bn.running_mean.is_contiguous()):
        raise ValueError("running statistics must be contiguous fp32")
    return _BNReLUTrainFn.apply(x, bn.weight, bn.bias, residual, bn, bool(relu), bool(passthrough))


class _AggregateFn(torch.autograd.Function):
    """softmax over supports -> label aggregation -> log(. + 1e-12) of a given score matrix (nw.py:285-289)."""

    @staticmethod
    def forward(ctx, scores, sy, n_classes):
        lib = _lib.load()
        sc = _f32c(scores)
        syc = _i64c(sy)
        B, N = sc.shape
        out = torch.empty(B, n_classes, dtype=torch.float32, device=sc.device)
        lse = torch.empty(B, dtype=torch.float32, device=sc.device)
        with _OnDevice(sc.device):
            _lib.check(lib.nw_aggregate_f32(_ptr(sc), _ptr(syc), _ptr(out), _ptr(lse), None, B, N, n_classes,
                                            int(syc.dim() == 2), _stream(sc)), "nw_aggregate_f32")
        ctx.save_for_backward(sc, syc, lse, out)
        ctx.C = n_classes
        return out

    @staticmethod
    def backward(ctx, gout):
        lib = _lib.load()
        sc, syc, lse, out = ctx.saved_tensors
        B, N = sc.shape
        g = _f32c(gout)
        gs = torch.empty_like(sc)
        with _OnDevice(sc.device):
            _lib.check(lib.nw_aggregate_bwd_f32(_ptr(sc), _ptr(syc), _ptr(lse), _ptr(out), _ptr(g), _ptr(gs), B, N, ctx.C,
                                                int(syc.dim() == 2), _stream(sc)), "nw_aggregate_bwd_f32")
        return gs, None, None


def nw_aggregate(scores, sy, n_classes):
    """(B,N) scores from ANY score function (on the device, possibly with a torch autograd history) + labels (N,) or
    (B,N) -> (B,C) log-probabilities: the softmax / label aggregation / log tail of NWHead.forward, differentiable
    with respect to the scores."""
    _need_hip(scores, sy)
    if scores.dim() != 2 or (sy.dim() == 1 and sy.shape[0] != scores.shape[1]) or (sy.dim() == 2 and sy.shape != scores.shape):
        raise ValueError("scores must be (B,N) and labels (N,) or (B,N)")
    return _AggregateFn.apply(scores, sy, int(n_classes))


def nw_head_influence(q, s, sy, n_classes, qy, kind="euclidean", logit_scale=None, support_cache=None):
    """NWHead.forward plus util/metric.py:23-50 on its own outputs in one call (no grad): returns
    (out (B,C) log-probabilities, infl (B,N)) with infl[b,j] = log((p - p*w_bj) / (p - w_bj*[sy_j == qy_b])),
    p = exp(out[b, qy_b]), w = the head's softmax weights -- which are never materialised: the tile kernel writes
    raw scores into the influence buffer and one in-place pass finishes them (nw_fwd_influence_f32).
    Shared (N,d) supports only."""
    _need_hip(q, s, sy, qy, logit_scale)
    kid = _kind_id(kind)
    if kid == SCORE_KINDS["clip"] and logit_scale is None:
        raise ValueError("clip kernel needs logit_scale")
    if s.dim() != 2 or sy.dim() != 1:
        raise ValueError("nw_head_influence takes a shared (N,d) support with (N,) labels")
    if support_cache is not None and not support_cache.matches(s):
        raise ValueError("support_cache was prepared from another support tensor")
    lib = _lib.load()
    # influences are indexed by support position; the call passes the default options (no run tables)
    call = _resolve(support_cache, _f32c(q), _f32c(s), sy, n_classes, positional=True, run_tables=False)
    qc, sc = call.q, call.s
    qyc = qy.detach().to(torch.int64).contiguous()
    B, d = qc.shape
    N, C = sc.shape[0], int(n_classes)
    if qyc.shape != (B,):
        raise ValueError("qy must be (B,)")
    dev = qc.device
    out = torch.empty(B, C, dtype=torch.float32, device=dev)
    infl = torch.empty(B, N, dtype=torch.float32, device=dev)
    ls = None if logit_scale is None else _f32c(logit_scale)
    st = _stream(qc)
    ws, ws_bytes = _fwd_workspace(lib, B, N, d, C, dev, st)
    with _OnDevice(dev):
        _lib.check(lib.nw_fwd_influence_f32(_ptr(qc), _ptr(sc), _ptr(call.sy), _ptr(call.norm2), _ptr(call.operand),
                                            _ptr(call.scale), _ptr(qyc), _ptr(out), None, _ptr(infl), _ptr(ws), ws_bytes, B, N,
                                            d, C, kid, _ptr(ls), call.opts, st), "nw_fwd_influence_f32")
    return out, infl


TopInfluence = collections.namedtuple("TopInfluence", "out helpful_rows helpful_infl harmful_rows harmful_infl")
INFLUENCE_SELECT_MAX_K = 32


def _influence_select(lib, vals, rows, sy, qy, out, lse, want_labels=False):
    """nw_influence_select_f32: the influences (and labels) of the (B,k) selected rows."""
    B, k = rows.shape
    infl = torch.empty(B, k, dtype=torch.float32, device=rows.device)
    labels = torch.empty(B, k, dtype=torch.int64, device=rows.device) if want_labels else None
    with _OnDevice(rows.device):
        _lib.check(lib.nw_influence_select_f32(_ptr(vals), _ptr(rows), _ptr(sy), _ptr(qy), _ptr(out), _ptr(lse), _ptr(infl),
                                               _ptr(labels), B, k, sy.shape[0], out.shape[1], _stream(rows)),
                   "nw_influence_select_f32")
    return (infl, labels) if want_labels else infl


def nw_top_influence(q, s, sy, n_classes, qy, k, kind="euclidean", logit_scale=None, support_cache=None,
                     return_labels=False):
    """The k most helpful and the k most harmful supports of every query, with their influences (util/metric.py:23-50),
    without the (B,N) influence matrix of nw_head_influence (no grad).  Returns TopInfluence(out (B,C) log-probabilities,
    helpful_rows, helpful_infl, harmful_rows, harmful_infl), each of the last four (B,k); rows are rows of `s`.

    infl[b,j] = log((p - p*w_bj) / (p - w_bj*[sy_j == qy_b])) grows with w over the supports of the query's own class
    (and is >= 0 there) and falls with w over the others (log(1 - w) <= 0): the most helpful supports are the best-scoring
    rows of class qy_b, the most harmful ones the best-scoring rows of the other classes.  With `sy` non-decreasing -- the
    bank NWNet.precompute() builds -- a class is one row range, so the two lists are two windowed searches
    (nw_knn(row_window=...), inside and excluded) and k influences each (nw_influence_select_f32), next to one forward for
    `out` and the log-sum-exp.  helpful_infl is non-increasing along k and harmful_infl non-decreasing (most harmful
    first); a list with fewer than k supports (a class of 3 rows) ends in row -1, influence 0.0.
    1 <= k <= 32.  support_cache: the SplitBank of `s` (one is built for the call otherwise); an fp16 bank is served
    through the fp32 rows, as every search over it is.  Unsorted `sy`: ValueError (nw_head_influence gives the matrix).
    return_labels: returns (TopInfluence, (helpful_labels, harmful_labels)), the (B,k) labels of the selected rows (-1 in
    an empty slot)."""
    _need_hip(q, s, sy, qy, logit_scale)
    kid = _kind_id(kind)
    if kid == SCORE_KINDS["clip"] and logit_scale is None:
        raise ValueError("clip kernel needs logit_scale")
    if s.dim() != 2 or sy.dim() != 1 or sy.shape[0] != s.shape[0]:
        raise ValueError("nw_top_influence takes a shared (N,d) support with (N,) labels")
    k = int(k)
    if not 1 <= k <= INFLUENCE_SELECT_MAX_K or k > s.shape[0]:
        raise NWHipError(f"nw_top_influence: k = {k} outside [1, min(N = {s.shape[0]}, {INFLUENCE_SELECT_MAX_K})]")
    syc = sy.detach().to(torch.int64).contiguous()
    if syc.numel() > 1 and bool((syc[1:] < syc[:-1]).any()):
        raise ValueError("nw_top_influence needs non-decreasing support labels (the class-sorted bank NWNet.precompute() "
                         "builds): a class must be one row range.  nw_head_influence gives the whole (B,N) influence "
                         "matrix for any label order")
    if support_cache is not None and not support_cache.matches(s):
        raise ValueError("support_cache was prepared from another support tensor")
    bank = support_cache if support_cache is not None else SplitBank(s, labels=sy)
    lib = _lib.load()
    qc, sc = _f32c(q), _f32c(s)
    B = qc.shape[0]
    qyc = qy.detach().to(torch.int64).contiguous()
    if qyc.shape != (B,):
        raise ValueError("qy must be (B,)")
    # one forward over the bank: the log-probabilities and the log-sum-exp of the scores (positional: the bank's rows as
    # they stand)
    call = _resolve(bank, qc, sc, sy, n_classes, positional=True)
    fq, fs = call.q, call.s
    N, C, dev = fs.shape[0], int(n_classes), qc.device
    out = torch.empty(B, C, dtype=torch.float32, device=dev)
    lse = torch.empty(B, dtype=torch.float32, device=dev)
    ls = None if logit_scale is None else _f32c(logit_scale)
    st = _stream(qc)
    ws, ws_bytes = _fwd_workspace(lib, B, N, fq.shape[1], C, dev, st)
    with _OnDevice(dev):
        _lib.check(lib.nw_fwd_f32(_ptr(fq), _ptr(fs), _ptr(call.sy), _ptr(call.norm2), _ptr(call.operand), _ptr(call.scale),
                                  _ptr(out), None, _ptr(lse), None, _ptr(ws), ws_bytes, B, N, fq.shape[1], C, kid, _ptr(ls),
                                  0, 0, call.opts, st), "nw_fwd_f32")
    # the rows of class qy_b, and the two searches
    window = (torch.searchsorted(syc, qyc), torch.searchsorted(syc, qyc, right=True))
    lists = []
    for exclude in (False, True):
        rows, vals = nw_knn(qc, bank, k, kind, logit_scale, return_values=True, support=sc, row_window=window,
                            exclude=exclude)
        lists.append((rows, _influence_select(lib, vals, rows, syc, qyc, out, lse, want_labels=return_labels)))
    (hr, hi), (br, bi) = lists
    if return_labels:
        return TopInfluence(out, hr, hi[0], br, bi[0]), (hi[1], bi[1])
    return TopInfluence(out, hr, hi, br, bi)


def support_influence_idx(probs, qy, w, sy):
    """Index-label form of util/metric.py:23-50: probs (B,C), qy (B,), w (B,N), sy (N,) -> (B,N)."""
    _need_hip(probs, qy, w, sy)
    lib = _lib.load()
    probs, w = _f32c(probs), _f32c(w)
    qy = qy.detach().to(torch.int64).contiguous()
    sy = sy.detach().to(torch.int64).contiguous()
    B, Cc = probs.shape
    N = w.shape[1]
    out = torch.empty(B, N, dtype=torch.float32, device=probs.device)
    with _OnDevice(probs.device):
        _lib.check(lib.nw_support_influence_f32(_ptr(probs), _ptr(qy), _ptr(w), _ptr(sy), _ptr(out), B, N, Cc,
                                                _stream(probs)), "nw_support_influence_f32")
    return out


# ------------------------------------------------------------------------------------------------------------------
# Convolutions on the fp16 matrix cores at fp32-grade accuracy (csrc/conv_nhwc.hip): fp32 channels_last activations,
# weights split once per update, activations split in flight with one power of two per tensor.
AMAX_SLOTS = 256    # floats of an `amax` record: per-workgroup partial maxima of its producer (their max bounds max|x|)


def absmax(x):
    """A bound on max |x| of a dense fp32 HIP tensor as an amax record -- AMAX_SLOTS partial maxima, no atomics, nothing to
    clear -- (nw_absmax_f32): what a tensor needs before it can feed conv2d_nhwc when its producer did not leave one."""
    _need_hip(x)
    xc = x if (x.dtype == torch.float32 and (x.is_contiguous() or x.is_contiguous(memory_format=torch.channels_last))) \
        else x.float().contiguous()
    out = torch.empty(AMAX_SLOTS, dtype=torch.float32, device=xc.device)
    with _OnDevice(xc.device):
        _lib.check(_lib.load().nw_absmax_f32(_ptr(xc), xc.numel(), _ptr(out), _stream(xc)), "nw_absmax_f32")
    return out


def to_nhwc_pad(x, cpad=4):
    """(n, c, h, w) fp32 HIP tensor, NCHW-contiguous or channels_last -> (n, cpad, h, w) channels_last with zero channels
    behind the c real ones, carrying `.nw_amax` (one pass: nw_to_nhwc_pad_f32).  What the stem convolution reads."""
    _need_hip(x)
    n, c, h, w = x.shape
    if x.dtype != torch.float32 or not (x.is_contiguous() or x.is_contiguous(memory_format=torch.channels_last)):
        x = x.float().contiguous()
    y = torch.empty((n, cpad, h, w), dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
    am = torch.empty(AMAX_SLOTS, dtype=torch.float32, device=x.device)
    with _OnDevice(x.device):
        _lib.check(_lib.load().nw_to_nhwc_pad_f32(_ptr(x), _ptr(y), _ptr(am), n, c, h * w, cpad, c * h * w, x.stride(1),
                                                  x.stride(3), _stream(x)), "nw_to_nhwc_pad_f32")
    y.nw_amax = am
    return y


class SplitConvWeight:
    """A (Cout, Cin, KH, KW) convolution weight prepared for conv2d_nhwc: its channels_last bytes are a (Cout,
    KH*KW*Cin) matrix whose rows go through nw_split_rows_f16x2 (one power of two per output channel).  Rebuild after
    every weight update."""

    def __init__(self, w):
        _need_hip(w)
        cout, cin, kh, kw = w.shape
        if cin == 3 and kw <= 8:        # RGB stems run on a 4-channel input (to_nhwc_pad): a pixel is one aligned float4
            w = torch.nn.functional.pad(w.detach(), (0, 0, 0, 0, 0, 1))
            cin = 4
        rows = w.detach().float().permute(0, 2, 3, 1).contiguous()          # (cout, kh, kw, cin)
        if cin % 32 == 0:
            rows = rows.view(cout, kh * kw * cin)
        elif kw * cin <= 32:
            # few input channels (the 7x7 stem over RGB): one kernel ROW is one 32-wide k chunk, zero-padded
            rows = torch.nn.functional.pad(rows.view(cout, kh, kw * cin), (0, 32 - kw * cin)).reshape(cout, kh * 32)
        else:
            raise ValueError("conv2d_nhwc needs Cin % 32 == 0 (or KW * Cin <= 32)")
        self.shape = (cout, cin, kh, kw)
        self.split = torch.empty_like(rows)
        self.scale = torch.empty(cout, dtype=torch.float32, device=rows.device)
        norm2 = torch.empty(cout, dtype=torch.float32, device=rows.device)
        with _OnDevice(rows.device):
            _lib.check(_lib.load().nw_split_rows_f16x2(_ptr(rows), _ptr(self.split), _ptr(self.scale), _ptr(norm2),
                                                       cout, rows.shape[1], _stream(rows)), "nw_split_rows_f16x2")


def conv2d_nhwc_supported(x_shape, w_shape, stride, pad):
    n, cin, h, w = x_shape
    cout, cin2, kh, kw = w_shape
    return cin == cin2 and bool(_lib.load().nw_conv2d_nhwc_supported(n, h, w, cin, cout, kh, kw, stride, pad))


def conv2d_nhwc(x, weight, bias=None, residual=None, relu=False, stride=1, pad=0, amax=None, want_amax=True, room=0):
    """y = post(conv2d(x, W, stride, pad) + bias [+ residual]) for a channels_last fp32 (n, Cin, H, W) HIP tensor and a
    SplitConvWeight; returns a channels_last (n, Cout, Ho, Wo) tensor.  `amax`: the amax record of x (AMAX_SLOTS floats
    whose maximum bounds max|x|; default: x.nw_amax when x came out of this function, else one absmax pass); the result
    carries its own in `.nw_amax` when want_amax.  room: channels to leave behind every pixel's Cout (_with_room)."""
    _need_hip(x, bias, residual)
    lib = _lib.load()
    n, cin, h, w = x.shape
    cout, cin2, kh, kw = weight.shape
    if cin == 3 and cin2 == 4:          # an RGB stem: SplitConvWeight padded its weight, the input follows (one pass, with amax)
        x = to_nhwc_pad(x, 4)
        cin = 4
    if cin != cin2:
        raise ValueError(f"conv2d_nhwc: input has {cin} channels, the weight {cin2}")
    if x.dtype != torch.float32 or not x.is_contiguous(memory_format=torch.channels_last):
        x = x.float().contiguous(memory_format=torch.channels_last)
    if amax is None:
        amax = getattr(x, "nw_amax", None)
        if amax is None:
            amax = absmax(x)
    ho, wo = (h + 2 * pad - kh) // stride + 1, (w + 2 * pad - kw) // stride + 1
    y, ldy = _with_room(n, cout, ho, wo, room, x.device)
    if residual is not None and (residual.shape != y.shape or residual.dtype != torch.float32
                                 or not residual.is_contiguous(memory_format=torch.channels_last)):
        residual = residual.float().expand_as(y).contiguous(memory_format=torch.channels_last)
    am_out = torch.empty(AMAX_SLOTS, dtype=torch.float32, device=x.device) if want_amax else None
    with _OnDevice(x.device):
        _lib.check(lib.nw_conv2d_nhwc_f16x2(_ptr(x), _ptr(amax), _ptr(weight.split), _ptr(weight.scale),
                                            None if bias is None else _ptr(_f32c(bias)), _ptr(residual), int(bool(relu)),
                                            _ptr(y), _ptr(am_out), n, h, w, cin, cout, kh, kw, int(stride), int(pad), 0,
                                            ldy if room > 0 else 0, None, _stream(x)), "nw_conv2d_nhwc_f16x2")
    if want_amax:
        y.nw_amax = am_out
    return y


STEM_POOL_FUSED = os.environ.get("NW_STEM_POOL_FUSED", "1") != "0"


@torch.no_grad()
def stem_conv_relu_maxpool_nhwc(x, weight, bias, room=0):
    """maxpool3x3/2/1(relu(conv7x7/2/3(x) + bias)) of an ImageNet stem at inference (model/resnet.py:147, :200-203,
    model/densenet.py:114-120; BatchNorm folded into `weight`, a SplitConvWeight of shape (64, 4, 7, 7), and `bias`) as ONE kernel
    (nw_stem7x7s2_relu_maxpool_f16x2) when it serves the shape, else the convolution and the pool; x: (n, 3, H, W) fp32 on the
    device.  The result is channels_last with `.nw_amax`; room: see conv2d_nhwc."""
    _need_hip(x, bias)
    lib = _lib.load()
    n, cin, h, w = x.shape
    cout = weight.shape[0]
    if not (STEM_POOL_FUSED and cin == 3 and tuple(weight.shape[1:]) == (4, 7, 7) and bias is not None
            and lib.nw_stem7x7s2_relu_maxpool_supported(n, h, w, cout)):
        return maxpool3s2_nhwc(conv2d_nhwc(x, weight, bias, None, True, 2, 3), room)
    x4 = to_nhwc_pad(x, 4)
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    hp, wp = (ho - 1) // 2 + 1, (wo - 1) // 2 + 1
    y, ldy = _with_room(n, cout, hp, wp, room, x.device)
    am = torch.empty(AMAX_SLOTS, dtype=torch.float32, device=x.device)
    with _OnDevice(x.device):
        _lib.check(lib.nw_stem7x7s2_relu_maxpool_f16x2(_ptr(x4), _ptr(x4.nw_amax), _ptr(weight.split), _ptr(weight.scale), _ptr(_f32c(bias)),
                                                       _ptr(y), _ptr(am), n, h, w, ldy if room > 0 else 0, _stream(x4)),
                   "nw_stem7x7s2_relu_maxpool_f16x2")
    y.nw_amax = am
    return y


# ------------------------------------------------------------------------------------------------------------------
# Channels-last training path: BatchNorm + ReLU (csrc/bn_nhwc.hip) and the convolution's autograd node.
def _nhwc_rows(x):
    """(n, c, h, w) fp32 HIP tensor whose memory is (n h w) rows of >= c floats (channels_last, or a channel prefix /
    window of a channels_last tensor) -> (tensor, row stride); anything else is made channels_last."""
    n, c, h, w = x.shape
    if x.dtype == torch.float32 and x.numel():
        ld = x.stride(3) if w > 1 else (x.stride(2) if h > 1 else (x.stride(0) if n > 1 else c))
        if (x.stride(1) == 1 and ld >= c and ld % 4 == 0 and (w == 1 or x.stride(3) == ld) and (h == 1 or x.stride(2) == w * ld)
                and (n == 1 or x.stride(0) == h * w * ld) and x.data_ptr() % 16 == 0):
            return x, ld
    x = x.float().contiguous(memory_format=torch.channels_last)
    return x, c


class _BNReLUNhwcFn(torch.autograd.Function):
    """relu(batch_norm(x)) in training mode over channels-last activations (nw_bn_relu_nhwc_train_fwd_f32 / _bwd_f32)."""

    @staticmethod
    def forward(ctx, x, weight, bias, bn, relu, passthrough=False):
        lib = _lib.load()
        xv, ldx = _nhwc_rows(x.detach())
        n, c, h, w = xv.shape
        rows = n * h * w
        dev = xv.device
        y = torch.empty((n, c, h, w), dtype=torch.float32, device=dev, memory_format=torch.channels_last)
        mean = torch.empty(c, dtype=torch.float32, device=dev)
        invstd = torch.empty_like(mean)
        amax = torch.empty(AMAX_SLOTS, dtype=torch.float32, device=dev)
        track = bn.track_running_stats and bn.running_mean is not None
        momentum, nbt = 0.0, None
        if track:
            if bn.momentum is None:
                bn.num_batches_tracked += 1
                momentum = 1.0 / float(bn.num_batches_tracked)
            else:
                momentum, nbt = float(bn.momentum), bn.num_batches_tracked
        wc, bc = _f32c(weight), _f32c(bias)
        ws_bytes = lib.nw_bn_nhwc_workspace_bytes(rows, c)
        ws = _workspace(ws_bytes, dev)
        with _OnDevice(dev):
            _lib.check(lib.nw_bn_relu_nhwc_train_fwd_f32(_ptr(xv), ldx, _ptr(wc), _ptr(bc),
                                                         _ptr(bn.running_mean) if track else None,
                                                         _ptr(bn.running_var) if track else None, _ptr(y), _ptr(mean),
                                                         _ptr(invstd), _ptr(nbt), _ptr(amax), _ptr(ws), ws_bytes, rows, c,
                                                         momentum, float(bn.eps), int(relu), _stream(xv)),
                       "nw_bn_relu_nhwc_train_fwd_f32")
        ctx.save_for_backward(xv, wc, bc, mean, invstd)
        ctx.relu, ctx.ldx, ctx.passthrough = relu, ldx, passthrough
        y.nw_amax = amax
        if passthrough:
            ctx.set_materialize_grads(False)
            return y, x.view_as(x)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy, gpass=None):
        lib = _lib.load()
        xv, wc, bc, mean, invstd = ctx.saved_tensors
        if gy is None:
            return gpass, None, None, None, None, None
        n, c, h, w = xv.shape
        rows = n * h * w
        dev = xv.device
        if gy.dtype != torch.float32 or not gy.is_contiguous(memory_format=torch.channels_last):
            gy = gy.float().contiguous(memory_format=torch.channels_last)
        acc, ldacc = None, 0
        if gpass is not None:
            acc, ldacc = _nhwc_rows(gpass)
        dx = torch.empty((n, c, h, w), dtype=torch.float32, device=dev, memory_format=torch.channels_last)
        dg, db = torch.empty_like(mean), torch.empty_like(mean)
        amax = torch.empty(AMAX_SLOTS, dtype=torch.float32, device=dev)
        ws_bytes = lib.nw_bn_nhwc_workspace_bytes(rows, c)
        ws = _workspace(ws_bytes, dev)
        with _OnDevice(dev):
            _lib.check(lib.nw_bn_relu_nhwc_train_bwd_f32(_ptr(xv), ctx.ldx, _ptr(gy), _ptr(wc), _ptr(bc), _ptr(mean), _ptr(invstd),
                                                         _ptr(dx), _ptr(dg), _ptr(db), _ptr(acc), ldacc, 0, _ptr(amax), _ptr(ws),
                                                         ws_bytes, rows, c, int(ctx.relu), _stream(xv)),
                       "nw_bn_relu_nhwc_train_bwd_f32")
        dx.nw_amax = amax
        dx.nw_fresh = True        # nobody else holds this buffer: a dense block's backward may use it as its gradient slab
        return dx, dg, db, None, None, None


BN_NHWC_MAX_C = 2560      # channels nw_bn_relu_nhwc_train_* serve (bn_nhwc.hip: BN_MAX_C)


def bn_relu_train_nhwc(x, bn, relu=True, passthrough=False):
    """relu(bn(x)) for a BatchNorm2d in training mode over a channels-last fp32 activation on the MI355X; the result is
    channels_last and carries `.nw_amax` for the convolution that follows.  passthrough: see bn_relu_train."""
    _need_hip(x, bn.weight, bn.bias)
    if not (bn.affine and bn.weight is not None):
        raise ValueError("bn_relu_train_nhwc needs an affine BatchNorm2d")
    if x.shape[0] * x.shape[2] * x.shape[3] <= 1:
        raise ValueError(f"Expected more than 1 value per channel when training, got input size {tuple(x.shape)}")
    if x.shape[1] % 4:
        raise ValueError("bn_relu_train_nhwc needs a channel count that is a multiple of 4")
    if x.shape[1] > BN_NHWC_MAX_C:           # wider than the kernels' per-channel tables: torch's BatchNorm on the same layout
        # (torch's own order: count first; momentum None = cumulative average with factor 1 / count, nn/modules/batchnorm.py)
        if bn.track_running_stats and bn.num_batches_tracked is not None:
            bn.num_batches_tracked += 1
        factor = bn.momentum
        if factor is None:
            factor = 1.0 / float(bn.num_batches_tracked) if (bn.track_running_stats and bn.num_batches_tracked is not None) else 0.0
        y = torch.nn.functional.batch_norm(x, bn.running_mean, bn.running_var, bn.weight, bn.bias, True, factor, bn.eps)
        y = torch.relu(y) if relu else y
        return (y, x) if passthrough else y
    return _BNReLUNhwcFn.apply(x, bn.weight, bn.bias, bn, bool(relu), bool(passthrough))


class _AddReluNhwcFn(torch.autograd.Function):
    """relu(a + b) over two channels-last tensors (the end of a residual block, model/resnet.py:60-66) with the amax record of the
    result; backward: ONE masked gradient for both summands (nw_add_relu_f32 / nw_relu_bwd_f32)."""

    @staticmethod
    def forward(ctx, a, b):
        lib = _lib.load()
        av, bv = a.detach(), b.detach()
        if not (av.is_contiguous(memory_format=torch.channels_last) and bv.is_contiguous(memory_format=torch.channels_last)):
            av, bv = av.contiguous(memory_format=torch.channels_last), bv.contiguous(memory_format=torch.channels_last)
        out = torch.empty_like(av, memory_format=torch.channels_last)
        amax = torch.empty(AMAX_SLOTS, dtype=torch.float32, device=av.device)
        with _OnDevice(av.device):
            _lib.check(lib.nw_add_relu_f32(_ptr(av), _ptr(bv), _ptr(out), _ptr(amax), av.numel(), _stream(av)), "nw_add_relu_f32")
        ctx.save_for_backward(out)
        out.nw_amax = amax
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        lib = _lib.load()
        out, = ctx.saved_tensors
        if g.dtype != torch.float32 or not g.is_contiguous(memory_format=torch.channels_last):
            g = g.float().contiguous(memory_format=torch.channels_last)
        dx = torch.empty_like(out, memory_format=torch.channels_last)
        amax = torch.empty(AMAX_SLOTS, dtype=torch.float32, device=out.device)
        with _OnDevice(out.device):
            _lib.check(lib.nw_relu_bwd_f32(_ptr(out), _ptr(g), _ptr(dx), _ptr(amax), out.numel(), _stream(out)), "nw_relu_bwd_f32")
        dx.nw_amax = amax
        return dx, dx


def add_relu_nhwc(a, b):
    """relu(a + b) for two channels-last fp32 activations of one shape on the MI355X; the result carries `.nw_amax`."""
    _need_hip(a, b)
    if a.shape != b.shape or a.dtype != torch.float32 or b.dtype != torch.float32 or a.numel() % 4:
        out = torch.relu(a + b)
        out.nw_amax = absmax(out.detach())
        return out
    return _AddReluNhwcFn.apply(a, b)


def _with_room(n, c, h, w, room, dev):
    """A channels-last (n, c, h, w) result tensor, alone or -- room > 0 -- as the first c channels of a fresh (n, c + room, h, w)
    allocation it carries as `.nw_slab`: a dense block that follows adopts that allocation as its slab instead of copying its
    input into one (_DenseBlockNhwcFn).  -> (tensor, row stride)"""
    if room <= 0:
        return torch.empty((n, c, h, w), dtype=torch.float32, device=dev, memory_format=torch.channels_last), c
    full = torch.empty((n, c + room, h, w), dtype=torch.float32, device=dev, memory_format=torch.channels_last)
    y = full[:, :c]
    y.nw_slab = full
    return y, c + room


class _AvgPool2NhwcFn(torch.autograd.Function):
    """F.avg_pool2d(x, 2, 2) over a channels-last fp32 activation (nw_avgpool2x2_nhwc_f32 / _bwd_f32)."""

    @staticmethod
    def forward(ctx, x, room):
        lib = _lib.load()
        xv, ldx = _nhwc_rows(x.detach())
        n, c, h, w = xv.shape
        y, ldy = _with_room(n, c, h // 2, w // 2, room, xv.device)
        with _OnDevice(xv.device):
            _lib.check(lib.nw_avgpool2x2_nhwc_f32(_ptr(xv), ldx, _ptr(y), ldy, n, h, w, c, _stream(xv)), "nw_avgpool2x2_nhwc_f32")
        ctx.shape = (n, c, h, w)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        lib = _lib.load()
        n, c, h, w = ctx.shape
        gv, ldg = _nhwc_rows(gy)
        gx = torch.empty((n, c, h, w), dtype=torch.float32, device=gv.device, memory_format=torch.channels_last)
        with _OnDevice(gv.device):
            _lib.check(lib.nw_avgpool2x2_nhwc_bwd_f32(_ptr(gv), ldg, _ptr(gx), c, n, h, w, c, _stream(gv)),
                       "nw_avgpool2x2_nhwc_bwd_f32")
        return gx, None


class _MaxPool3s2NhwcFn(torch.autograd.Function):
    """F.max_pool2d(x, 3, 2, 1) over a channels-last fp32 activation (nw_maxpool3x3s2_nhwc_f32 / _bwd_f32): the winning tap of
    each window is kept as one byte for the backward."""

    @staticmethod
    def forward(ctx, x, room):
        lib = _lib.load()
        xv, ldx = _nhwc_rows(x.detach())
        n, c, h, w = xv.shape
        ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        y, ldy = _with_room(n, c, ho, wo, room, xv.device)
        tap = torch.empty((n, ho, wo, c), dtype=torch.uint8, device=xv.device)
        with _OnDevice(xv.device):
            _lib.check(lib.nw_maxpool3x3s2_nhwc_f32(_ptr(xv), ldx, _ptr(y), ldy, _ptr(tap), n, h, w, c, _stream(xv)),
                       "nw_maxpool3x3s2_nhwc_f32")
        ctx.save_for_backward(tap)
        ctx.shape = (n, c, h, w)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        lib = _lib.load()
        tap, = ctx.saved_tensors
        n, c, h, w = ctx.shape
        gv, ldg = _nhwc_rows(gy)
        gx = torch.empty((n, c, h, w), dtype=torch.float32, device=gv.device, memory_format=torch.channels_last)
        with _OnDevice(gv.device):
            _lib.check(lib.nw_maxpool3x3s2_nhwc_bwd_f32(_ptr(gv), ldg, _ptr(tap), _ptr(gx), c, n, h, w, c, _stream(gv)),
                       "nw_maxpool3x3s2_nhwc_bwd_f32")
        return gx, None


def avgpool2_nhwc(x, room=0):
    """nn.AvgPool2d(2, 2) of a DenseNet transition (reference model/densenet.py:83-91) over a channels-last fp32 activation on
    the MI355X; the result is channels_last.  room: channels to leave behind every pixel's c (see _with_room)."""
    _need_hip(x)
    if x.dim() != 4 or x.shape[1] % 4 or x.shape[2] < 2 or x.shape[3] < 2:
        raise ValueError(f"avgpool2_nhwc needs (n, c % 4 == 0, h >= 2, w >= 2), got {tuple(x.shape)}")
    y = _AvgPool2NhwcFn.apply(x, int(room))
    if hasattr(x, "nw_amax"):           # an average is no larger than the largest value averaged: x's bound holds for y
        y.nw_amax = x.nw_amax
    return y


def maxpool3s2_nhwc(x, room=0):
    """nn.MaxPool2d(3, 2, 1) of the stems (reference model/densenet.py:114, model/resnet.py:147) over a channels-last fp32
    activation on the MI355X; the result is channels_last and keeps x's `.nw_amax` bound."""
    _need_hip(x)
    if x.dim() != 4 or x.shape[1] % 4:
        raise ValueError(f"maxpool3s2_nhwc needs (n, c % 4 == 0, h, w), got {tuple(x.shape)}")
    if not (torch.is_grad_enabled() and x.requires_grad):       # inference: no tap record
        xv, ldx = _nhwc_rows(x.detach())
        n, c, h, w = xv.shape
        y, ldy = _with_room(n, c, (h - 1) // 2 + 1, (w - 1) // 2 + 1, int(room), xv.device)
        with _OnDevice(xv.device):
            _lib.check(_lib.load().nw_maxpool3x3s2_nhwc_f32(_ptr(xv), ldx, _ptr(y), ldy, None, n, h, w, c, _stream(xv)),
                       "nw_maxpool3x3s2_nhwc_f32")
    else:
        y = _MaxPool3s2NhwcFn.apply(x, int(room))
    if hasattr(x, "nw_amax"):
        y.nw_amax = x.nw_amax
    return y


class _WeightOperand:
    """A split-row convolution operand inside a ConvWeightBank (the interface conv2d_nhwc reads: split, scale, shape)."""
    __slots__ = ("split", "scale", "shape")

    def __init__(self, split, scale, shape):
        self.split, self.scale, self.shape = split, scale, shape


class ConvWeightBank:
    """The split-row operands of ALL convolution weights of a network -- forward and, for stride-1 convolutions whose input
    needs a gradient, data-gradient (flipped taps, transposed channels) -- kept in two flat buffers and rebuilt by ONE
    launch (nw_split_conv_weights_f16x2) whenever a weight has changed since the last build (an optimizer step)."""

    def __init__(self, convs):
        """convs: list of (weight parameter (Cout, Cin, KH, KW), needs_dgrad)."""
        self.weights = [w for w, _ in convs]
        self._want = [bool(d) for _, d in convs]
        self._sig = None
        self._build_tables()

    def _build_tables(self):
        dev = self.weights[0].device
        jobs, views = [], []
        off = soff = rows_total = 0
        for w, want_dgrad in zip(self.weights, self._want):
            cout, cin, kh, kw = w.shape
            t = kh * kw
            if not (w.is_contiguous() and w.dtype == torch.float32):
                raise ValueError("ConvWeightBank needs contiguous fp32 weights")
            entry = [None, None]
            if cin % 32 == 0:
                rows, cols, mode, shape = cout, t * cin, 0, (cout, cin, kh, kw)
            elif cin <= 4 and kw * 4 <= 32:
                rows, cols, mode, shape = cout, kh * 32, 2, (cout, 4, kh, kw)
            else:
                rows = None
            if rows is not None:
                jobs.append([w.data_ptr(), off, soff, rows_total, rows, cols, cin, cout, t, kw | (mode << 32)])
                entry[0] = (off, soff, rows, cols, shape)
                off, soff, rows_total = off + rows * cols, soff + rows, rows_total + rows
            if want_dgrad and cin % 32 == 0 and cout % 32 == 0:
                rows, cols = cin, t * cout
                jobs.append([w.data_ptr(), off, soff, rows_total, rows, cols, cin, cout, t, kw | (1 << 32)])
                entry[1] = (off, soff, rows, cols, (cin, cout, kh, kw))
                off, soff, rows_total = off + rows * cols, soff + rows, rows_total + rows
            views.append(entry)
        self.split = torch.empty(max(off, 4), dtype=torch.float32, device=dev)
        self.scale = torch.empty(max(soff, 4), dtype=torch.float32, device=dev)
        self.jobs = torch.tensor(jobs, dtype=torch.int64).to(dev)
        self.total_rows = rows_total
        self._ops = {}
        for w, entry in zip(self.weights, views):
            made = []
            for e in entry:
                if e is None:
                    made.append(None)
                else:
                    o_, so_, rows, cols, shape = e
                    made.append(_WeightOperand(self.split[o_:o_ + rows * cols].view(rows, cols), self.scale[so_:so_ + rows], shape))
            self._ops[id(w)] = tuple(made)
        self._ptrs = tuple(w.data_ptr() for w in self.weights)

    def refresh(self, force=False):
        """Rebuild the operands if any weight changed (in place: its version; replaced: its address).  force: rebuild
        regardless -- what a training forward asks for, because torch's FUSED optimizers (SGD / Adam(fused=True)) update
        parameters without advancing their version counters, so an unchanged version proves nothing there."""
        ptrs = tuple(w.data_ptr() for w in self.weights)
        if ptrs != self._ptrs:
            self._build_tables()
            self._sig = None
        sig = tuple(_ver(w) for w in self.weights)
        if sig == self._sig and not force:
            return
        dev = self.split.device
        with _OnDevice(dev):
            _lib.check(_lib.load().nw_split_conv_weights_f16x2(_ptr(self.jobs), self.jobs.shape[0], self.total_rows,
                                                               _ptr(self.split), _ptr(self.scale), _stream(self.split)),
                       "nw_split_conv_weights_f16x2")
        self._sig = sig

    def has(self, w):
        return id(w) in self._ops

    def operands(self, w):
        """(forward operand, data-gradient operand or None) of weight parameter w."""
        return self._ops[id(w)]


_CONV_STATS = {"absmax_fallbacks": 0}


def _amax_of(t):
    """The amax record a tensor carries (conv2d_nhwc / bn_relu_train_nhwc leave one on their results), else one pass."""
    a = getattr(t, "nw_amax", None)
    if a is None:
        _CONV_STATS["absmax_fallbacks"] += 1
        a = absmax(t)
    return a


# Data and weight gradients of STRIDED many-channel convolutions (the ResNets' 3x3 / 2 and 1x1 / 2) on the own kernels: the data
# gradient as the stride-1 one over gy with zeros between its pixels, the weight gradient as one 1x1 problem per tap
# (round 4).  0: torch / MIOpen.
OWN_STRIDED_GRADS = os.environ.get("NW_OWN_STRIDED_GRADS", "1") != "0"


class _ConvNhwcFn(torch.autograd.Function):
    """conv2d over channels-last activations on the fp16 matrix cores: forward and data gradient through
    nw_conv2d_nhwc_f16x2 (the data gradient of a stride-1 convolution is the convolution with the flipped, transposed
    weight and padding k - 1 - p), weight gradient through nw_conv2d_nhwc_wgrad_f16x2 when it serves the shape."""

    @staticmethod
    def forward(ctx, x, weight, stride, pad, amax, operands, room=0):
        xv = x.detach()
        if xv.dtype != torch.float32 or not xv.is_contiguous(memory_format=torch.channels_last):
            xv = xv.float().contiguous(memory_format=torch.channels_last)
        fw = operands[0] if operands is not None and operands[0] is not None else SplitConvWeight(weight)
        if amax is None and not (xv.shape[1] == 3 and fw.shape[1] == 4):   # (an RGB stem gets its record from the padding pass)
            amax = _amax_of(x)
        y = conv2d_nhwc(xv, fw, None, None, False, stride, pad, amax=amax, room=room)
        ctx.save_for_backward(xv, weight, amax if amax is not None else torch.empty(0, device=xv.device))
        ctx.stride, ctx.pad = stride, pad
        ctx.dgrad_operand = operands[1] if operands is not None else None
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        xv, weight, amax_x = ctx.saved_tensors
        stride, pad = ctx.stride, ctx.pad
        cout, cin, kh, kw = weight.shape
        g = gy
        gam = getattr(gy, "nw_amax", None)
        if g.dtype != torch.float32 or not g.is_contiguous(memory_format=torch.channels_last):
            g = g.float().contiguous(memory_format=torch.channels_last)
        if gam is None:
            _CONV_STATS["absmax_fallbacks"] += 1
            gam = absmax(g)
        dx = dw = None
        if ctx.needs_input_grad[0]:
            if stride == 1 and kh == kw and kh - 1 - pad >= 0 and cout % 32 == 0 and cin % 32 == 0:
                dg = ctx.dgrad_operand
                if dg is None:
                    dg = SplitConvWeight(weight.detach().flip(2, 3).transpose(0, 1))     # (cin, cout, kh, kw)
                dx = conv2d_nhwc(g, dg, None, None, False, 1, kh - 1 - pad, amax=gam)
            elif (OWN_STRIDED_GRADS and stride > 1 and kh == kw and kh - 1 - pad >= 0 and cout % 32 == 0 and cin % 32 == 0
                  and xv.shape[2] + 2 * pad - kh + 1 >= (g.shape[2] - 1) * stride + 1):
                # strided: the stride-1 data gradient of gy with zeros between its pixels (model/resnet.py's 3x3 / 2 and 1x1 / 2
                # convolutions; three quarters of the products are with zeros -- six small layers of a ResNet)
                dg = ctx.dgrad_operand
                if dg is None:
                    dg = SplitConvWeight(weight.detach().flip(2, 3).transpose(0, 1))
                hd, wd = xv.shape[2] + 2 * pad - kh + 1, xv.shape[3] + 2 * pad - kw + 1
                gd = torch.zeros((g.shape[0], cout, hd, wd), dtype=torch.float32, device=g.device).contiguous(memory_format=torch.channels_last)
                gd[:, :, 0:(g.shape[2] - 1) * stride + 1:stride, 0:(g.shape[3] - 1) * stride + 1:stride] = g
                dx = conv2d_nhwc(gd, dg, None, None, False, 1, kh - 1 - pad, amax=gam)
            else:
                dx = torch.ops.aten.convolution_backward(g, xv, weight, None, [stride, stride], [pad, pad], [1, 1], False,
                                                         [0, 0], 1, [True, False, False])[0]
        if ctx.needs_input_grad[1]:
            dw = conv2d_nhwc_wgrad(xv, g, weight.shape, stride, pad, amax_x if amax_x.numel() else None, gam)
        return dx, dw, None, None, None, None, None


def conv2d_nhwc_wgrad(x, gy, wshape, stride, pad, amax_x=None, amax_g=None):
    """Weight gradient of conv2d for channels-last x (n, Cin, H, W) and gy (n, Cout, Ho, Wo) -> (Cout, Cin, KH, KW)
    (channels_last strides).  Stride-1 'same' 1x1 / 3x3 shapes run in nw_conv2d_nhwc_wgrad_f16x2; the rest (the strided
    stem) goes to MIOpen through torch."""
    lib = _lib.load()
    cout, cin, kh, kw = wshape
    n, _, h, w = x.shape
    if lib.nw_conv2d_nhwc_wgrad_supported(n, h, w, cin, cout, kh, kw, stride, pad):
        if amax_x is None:
            amax_x = _amax_of(x)
        if amax_g is None:
            amax_g = _amax_of(gy)
        dw = torch.empty((cout, kh, kw, cin), dtype=torch.float32, device=x.device)
        ws_bytes = lib.nw_conv2d_nhwc_wgrad_workspace_bytes(n, h, w, cin, cout, kh, kw, stride, pad)
        ws = _workspace(ws_bytes, x.device)
        with _OnDevice(x.device):
            _lib.check(lib.nw_conv2d_nhwc_wgrad_f16x2(_ptr(x), _ptr(amax_x), _ptr(gy), _ptr(amax_g), _ptr(dw), _ptr(ws), ws_bytes,
                                                      n, h, w, cin, cout, kh, kw, stride, pad, 0, 0, _stream(x)),
                       "nw_conv2d_nhwc_wgrad_f16x2")
        if kh == 1 and kw == 1:
            return dw.view(cout, cin, 1, 1)      # the same bytes in torch's own strides: AccumulateGrad takes it without a copy
        return dw.permute(0, 3, 1, 2)
    if cin == 3 and 4 * kw <= 32 and cout % 8 == 0 and x.is_cuda:
        # The few-channel stems (7x7 / 2 over RGB, model/densenet.py:114-116, model/resnet.py:147; round 4, VERDICT r03 item 3c:
        # MIOpen's igemm_wrw kernel was the last vendor kernel in K4's trace, with a 5 s solver search on a process's first
        # step): ONE 1x1 weight gradient between gy and, per kernel row, the 32-float run that row reads from the 4-channel
        # padded input (nw_wgrad_job.rowrun_stride: 32 KH "channels").
        x4 = to_nhwc_pad(x, 4)
        ho, wo = gy.shape[2], gy.shape[3]
        if amax_g is None:
            amax_g = _amax_of(gy)
        gyc = gy if gy.is_contiguous(memory_format=torch.channels_last) else gy.contiguous(memory_format=torch.channels_last)
        rows = torch.empty((cout, kh * 32), dtype=torch.float32, device=x.device)
        jobs = (_lib.WgradJob * 1)(_lib.WgradJob(_ptr(x4), _ptr(x4.nw_amax), _ptr(gyc), _ptr(amax_g), _ptr(rows), n, ho, wo, 32 * kh, cout,
                                                 1, 1, 1, 0, 0, 0, 0, None, int(stride), h, w, -pad, -pad))
        wsb = lib.nw_conv2d_nhwc_wgrad_batch_workspace_bytes(jobs, 1)
        ws = _workspace(wsb, x.device)
        with _OnDevice(x.device):
            _lib.check(lib.nw_conv2d_nhwc_wgrad_batch_f16x2(jobs, 1, _ptr(ws), wsb, _stream(x)), "nw_conv2d_nhwc_wgrad_batch_f16x2")
        # rows[co, 32 ky + 4 kx + ci] -> (cout, cin, kh, kw)
        return rows.view(cout, kh, 8, 4)[:, :, :kw, :3].permute(0, 3, 1, 2)
    if OWN_STRIDED_GRADS and stride > 1 and cin % 8 == 0 and cout % 8 == 0 and x.is_cuda and \
            lib.nw_conv2d_nhwc_wgrad_supported(n, gy.shape[2], gy.shape[3], cin, cout, 1, 1, 1, 0):
        # strided convolutions with many channels (model/resnet.py:31-66: 3x3 / 2, 1x1 / 2): one 1x1 problem per tap between gy
        # and the input pixels that tap reads (a strided slice of the padded input, copied densely), batched into one launch
        ho, wo = gy.shape[2], gy.shape[3]
        if amax_x is None:
            amax_x = _amax_of(x)
        if amax_g is None:
            amax_g = _amax_of(gy)
        gyc = gy if gy.is_contiguous(memory_format=torch.channels_last) else gy.contiguous(memory_format=torch.channels_last)
        xp = torch.nn.functional.pad(x, (pad, pad, pad, pad)) if pad else x
        taps = [xp[:, :, ky:ky + stride * (ho - 1) + 1:stride, kx:kx + stride * (wo - 1) + 1:stride].contiguous(memory_format=torch.channels_last)
                for ky in range(kh) for kx in range(kw)]
        dwt = torch.empty((kh * kw, cout, cin), dtype=torch.float32, device=x.device)
        jl = [_lib.WgradJob(_ptr(t), _ptr(amax_x), _ptr(gyc), _ptr(amax_g), dwt.data_ptr() + 4 * k * cout * cin, n, ho, wo, cin, cout,
                            1, 1, 1, 0, 0, 0, 0, None) for k, t in enumerate(taps)]
        jobs = (_lib.WgradJob * len(jl))(*jl)
        wsb = lib.nw_conv2d_nhwc_wgrad_batch_workspace_bytes(jobs, len(jl))
        ws = _workspace(wsb, x.device)
        with _OnDevice(x.device):
            _lib.check(lib.nw_conv2d_nhwc_wgrad_batch_f16x2(jobs, len(jl), _ptr(ws), wsb, _stream(x)), "nw_conv2d_nhwc_wgrad_batch_f16x2")
        del taps
        return dwt.permute(1, 2, 0).reshape(cout, cin, kh, kw) if kh * kw > 1 else dwt.view(cout, cin, 1, 1)
    # other strided shapes: MIOpen's channels-last weight-gradient kernel on channels-last operands (as NCHW tensors it copies
    # gy and transposes it back)
    return torch.ops.aten.convolution_backward(gy.contiguous(memory_format=torch.channels_last),
                                               x.contiguous(memory_format=torch.channels_last),
                                               torch.empty(wshape, dtype=x.dtype, device=x.device),
                                               None, [stride, stride], [pad, pad], [1, 1], False, [0, 0], 1,
                                               [False, True, False])[1]


def _bn_tracking(bn):
    """(running_mean, running_var, momentum, num_batches_tracked) as nw_bn_relu_nhwc_train_fwd_f32 takes them."""
    if not (bn.track_running_stats and bn.running_mean is not None):
        return None, None, 0.0, None
    if bn.momentum is None:
        bn.num_batches_tracked += 1
        return bn.running_mean, bn.running_var, 1.0 / float(bn.num_batches_tracked), None
    return bn.running_mean, bn.running_var, float(bn.momentum), bn.num_batches_tracked


class _DenseBlockNhwcFn(torch.autograd.Function):
    """A whole dense block (model/densenet.py:62-80: every layer reads the concatenation of the block's input and all
    earlier layers' outputs) as ONE autograd node over ONE slab: the block's output tensor (rows = n h w, C0 + L growth
    floats per row) is allocated once, the input is copied into its first C0 channels, and every layer's 3x3 convolution
    writes its `growth` channels into place (row stride = the slab's width), so no concatenation is ever made; norm1 of a
    layer reads a channel prefix of the slab.  The backward keeps ONE gradient slab: a layer's gradient is a channel window
    of it, and norm1's backward kernel adds its dx into the prefix in place -- the O(L^2) gradient accumulations and slice
    copies autograd derives for the concatenations do not exist.  Same kernels and arithmetic as the layer-by-layer path
    (ops.bn_relu_train_nhwc, ops.conv2d_nhwc_train); parameter gradients in the order of `params`:
    per layer norm1.weight, norm1.bias, conv1.weight, norm2.weight, norm2.bias, conv2.weight."""

    @staticmethod
    def forward(ctx, x, layers, bank, *params):
        lib = _lib.load()
        xv, ldx0 = _nhwc_rows(x.detach())
        n, c0, h, w = xv.shape
        rows, dev = n * h * w, xv.device
        L = len(layers)
        growth = layers[0].conv2.weight.shape[0]
        mid = layers[0].conv1.weight.shape[0]
        ctot = c0 + L * growth
        slab = getattr(x, "nw_slab", None)            # the producer left room behind x's channels (_with_room): no copy
        if not (slab is not None and tuple(slab.shape) == (n, ctot, h, w) and slab.data_ptr() == xv.data_ptr() and ldx0 == ctot
                and slab.dtype == torch.float32 and slab.is_contiguous(memory_format=torch.channels_last)):
            slab = torch.empty((n, ctot, h, w), dtype=torch.float32, device=dev, memory_format=torch.channels_last)
            slab[:, :c0] = xv
        st = _stream(xv)
        saved, meta = [], []
        f32 = dict(dtype=torch.float32, device=dev)
        eps = float(layers[0].norm1.eps)
        # Batch statistics per slab channel, computed ONCE: a channel's mean and variance are the same for every later layer's
        # norm1, the block's input channels get one pass here, and each convolution leaves the moments of the channels it writes
        # (nw_conv2d_nhwc_f16x2's `moments`), so no BatchNorm of the block reads its input for statistics.
        bstat = torch.empty(5 * ctot, **f32)                       # mean | invstd | var | min | max of the slab's channels
        bm, bi, bv, blo, bhi = (bstat[k * ctot:(k + 1) * ctot] for k in range(5))
        with _OnDevice(dev):
            wsb = lib.nw_bn_nhwc_minmax_workspace_bytes(rows, c0)
            ws = _workspace(wsb, dev)
            _lib.check(lib.nw_bn_nhwc_moments_minmax_f32(_ptr(slab), ctot, rows, c0, eps, _ptr(bm), _ptr(bi), _ptr(bv), _ptr(blo),
                                                         _ptr(bhi), _ptr(ws), wsb, st), "nw_bn_nhwc_moments_minmax_f32")
            def layer_params(k):
                g1, b1, w1, g2, b2, w2 = (t.detach() for t in params[6 * k:6 * k + 6])
                return _f32c(g1), _f32c(b1), w1, _f32c(g2), _f32c(b2), w2
            # Round 4: neither t1 = relu(norm1(prefix)) nor t2 = relu(norm2(u)) exists: the convolutions' loaders apply the
            # BatchNorm + ReLU on the way into LDS (nw_conv2d_nhwc_bnrelu_f16x2) from a per-channel table mean | a | beta, with
            # the exact bound on the transformed tensor (from each channel's minimum and maximum, which the producing
            # convolution's epilogue leaves beside the moments) as its amax record.  The table of a layer's norm1 is written by
            # the launch that merges the previous layer's fresh channels (nw_bn_nhwc_prep_window_from_partials_f32): four
            # launches per layer -- conv1, merge + norm2's table, conv2, merge + the next norm1's table.
            g1, b1, w1, g2, b2, w2 = layer_params(0)
            tab1 = torch.empty(3 * c0, **f32)
            am1 = torch.empty(AMAX_SLOTS, **f32)
            rm, rv, mom, nbt = _bn_tracking(layers[0].norm1)
            _lib.check(lib.nw_bn_nhwc_prep_f32(_ptr(bm), _ptr(bi), _ptr(bv), _ptr(blo), _ptr(bhi), _ptr(g1), _ptr(b1), _ptr(rm), _ptr(rv),
                                               _ptr(nbt), mom, 1, rows, c0, _ptr(tab1), _ptr(am1), st), "nw_bn_nhwc_prep_f32")
            for k, layer in enumerate(layers):
                c = c0 + k * growth
                o1, o2 = bank.operands(layer.conv1.weight), bank.operands(layer.conv2.weight)
                kh = w2.shape[2]
                u = torch.empty((rows, mid), **f32)
                stats = torch.empty(5 * mid, **f32)                        # norm2: mean | invstd | var | min | max
                tab2 = torch.empty(3 * mid, **f32)
                am2 = torch.empty(AMAX_SLOTS, **f32)                       # amax record of relu(norm2(u)) (am1: of relu(norm1(prefix)))
                m2, i2, v2, lo2, hi2 = (stats[j * mid:(j + 1) * mid] for j in range(5))
                G1 = lib.nw_conv2d_nhwc_moments_groups(n, h, w, c, mid, 1, 1, 1, 0)
                G2 = lib.nw_conv2d_nhwc_moments_groups(n, h, w, mid, growth, kh, kh, 1, kh // 2)
                part = _workspace(4 * 5 * max(G1 * mid, G2 * growth), dev)
                _lib.check(lib.nw_conv2d_nhwc_bnrelu_f16x2(_ptr(slab), _ptr(tab1), _ptr(am1), 0, _ptr(o1[0].split), _ptr(o1[0].scale), None, 0,
                                                           _ptr(u), None, n, h, w, c, mid, 1, 1, 1, 0, ctot, 0, _ptr(part), st),
                           "nw_conv2d_nhwc_bnrelu_f16x2")
                rm, rv, mom, nbt = _bn_tracking(layer.norm2)
                _lib.check(lib.nw_bn_nhwc_prep_from_partials_f32(_ptr(part), G1, mid, eps, _ptr(m2), _ptr(i2), _ptr(v2), _ptr(lo2),
                                                                 _ptr(hi2), _ptr(g2), _ptr(b2), _ptr(rm), _ptr(rv), _ptr(nbt), mom, 1,
                                                                 _ptr(tab2), _ptr(am2), st), "nw_bn_nhwc_prep_from_partials_f32")
                _lib.check(lib.nw_conv2d_nhwc_bnrelu_f16x2(_ptr(u), _ptr(tab2), _ptr(am2), 0, _ptr(o2[0].split), _ptr(o2[0].scale), None, 0,
                                                           slab.data_ptr() + 4 * c, None, n, h, w, mid, growth, kh, kh, 1, kh // 2, 0,
                                                           ctot, _ptr(part), st), "nw_conv2d_nhwc_bnrelu_f16x2")
                saved += [u, stats, tab1, am1, tab2, am2, g1, b1, g2, b2]
                meta.append((c, kh, o1[1], o2[1], tuple(w1.shape), tuple(w2.shape)))
                if k + 1 < L:      # the fresh channels' statistics + the whole table of the next layer's norm1
                    g1, b1, w1, g2, b2, w2 = layer_params(k + 1)
                    tab1 = torch.empty(3 * (c + growth), **f32)
                    am1 = torch.empty(AMAX_SLOTS, **f32)
                    rm, rv, mom, nbt = _bn_tracking(layers[k + 1].norm1)
                    _lib.check(lib.nw_bn_nhwc_prep_window_from_partials_f32(
                        _ptr(part), G2, growth, c, c, rows, eps, _ptr(bm), _ptr(bi), _ptr(bv), _ptr(blo), _ptr(bhi), _ptr(g1), _ptr(b1),
                        _ptr(rm), _ptr(rv), _ptr(nbt), mom, 1, _ptr(tab1), _ptr(am1), st), "nw_bn_nhwc_prep_window_from_partials_f32")
                else:
                    _lib.check(lib.nw_bn_nhwc_prep_window_from_partials_f32(
                        _ptr(part), G2, growth, c, 0, rows, eps, _ptr(bm), _ptr(bi), _ptr(bv), _ptr(blo), _ptr(bhi), None, None, None,
                        None, None, 0.0, 1, None, None, st), "nw_bn_nhwc_prep_window_from_partials_f32")
        saved.append(bstat)
        ctx.save_for_backward(slab, *saved)
        ctx.meta, ctx.dims = meta, (n, c0, h, w, growth, mid, ctot)
        return slab

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        lib = _lib.load()
        slab, *saved = ctx.saved_tensors
        bstat = saved[-1]
        n, c0, h, w, growth, mid, ctot = ctx.dims
        rows, dev = n * h * w, slab.device
        am_g = getattr(gout, "nw_amax", None)
        G = gout.float().contiguous(memory_format=torch.channels_last)
        if G.data_ptr() == gout.data_ptr() and not getattr(gout, "nw_fresh", False):
            G = G.clone(memory_format=torch.channels_last)             # the gradient slab is updated in place: a buffer of
                                                                       #   our own BatchNorm backward (`nw_fresh`) is adopted
        if am_g is None:
            am_g = absmax(G)
        st = _stream(slab)
        f32 = dict(dtype=torch.float32, device=dev)
        grads = [None] * (6 * len(ctx.meta))
        # the weight gradients are not on the critical path: collected here and run together behind the loop
        # (nw_conv2d_nhwc_wgrad_batch_f16x2: a dozen workgroups per 14x14 / 7x7 layer fill the chip only together)
        wjobs, wkeep = [], []
        with _OnDevice(dev):
            for k in range(len(ctx.meta) - 1, -1, -1):
                c, kh, d1, d2, w1s, w2s = ctx.meta[k]
                u, stats, tab1, am1, tab2, am2, g1, b1, g2, b2 = saved[10 * k:10 * k + 10]
                m1, i1, m2, i2 = bstat[:c], bstat[ctot:ctot + c], stats[:mid], stats[mid:2 * mid]
                # (tab1 / tab2: the forward's tables -- the weight gradients' x operands are relu(norm(.)) again, applied by
                #  THEIR loaders)
                gv = G.data_ptr() + 4 * c                              # this layer's window of the gradient slab
                # conv2 (3x3): weight gradient, data gradient
                dw2 = torch.empty((growth, mid, kh, kh), **f32)          # torch's layout: autograd takes it without a copy
                wjobs.append(_lib.WgradJob(_ptr(u), _ptr(am2), gv, _ptr(am_g), _ptr(dw2),
                                           n, h, w, mid, growth, kh, kh, 1, kh // 2, 0, ctot, 1, _ptr(tab2)))
                wkeep.append(am_g)
                dt2 = torch.empty((rows, mid), **f32)
                am_d = torch.empty(3 * AMAX_SLOTS, **f32)              # amax records of dt2 | du | dt1
                _lib.check(lib.nw_conv2d_nhwc_f16x2(gv, _ptr(am_g), _ptr(d2.split), _ptr(d2.scale), None, None, 0, _ptr(dt2),
                                                    _ptr(am_d), n, h, w, growth, mid, kh, kh, 1, kh - 1 - kh // 2, ctot, 0, None, st),
                           "nw_conv2d_nhwc_f16x2")
                # norm2 + relu
                du = torch.empty((rows, mid), **f32)
                dg2, db2 = torch.empty(mid, **f32), torch.empty(mid, **f32)
                bnb = max(lib.nw_bn_nhwc_workspace_bytes(rows, c), lib.nw_bn_nhwc_workspace_bytes(rows, mid))
                wsn = _workspace(bnb, dev)
                _lib.check(lib.nw_bn_relu_nhwc_train_bwd_f32(_ptr(u), mid, _ptr(dt2), _ptr(g2), _ptr(b2), _ptr(m2), _ptr(i2),
                                                             _ptr(du), _ptr(dg2), _ptr(db2), None, 0, 0,
                                                             am_d.data_ptr() + 4 * AMAX_SLOTS, _ptr(wsn), bnb, rows, mid, 1, st),
                           "nw_bn_relu_nhwc_train_bwd_f32")
                # conv1 (1x1)
                dw1 = torch.empty((mid, c, 1, 1), **f32)     # (a 1x1 kernel: (Cout, 1, 1, Cin) bytes ARE torch's (Cout, Cin, 1, 1): no copy in AccumulateGrad)
                wjobs.append(_lib.WgradJob(_ptr(slab), _ptr(am1), _ptr(du), am_d.data_ptr() + 4 * AMAX_SLOTS, _ptr(dw1),
                                           n, h, w, c, mid, 1, 1, 1, 0, ctot, 0, 0, _ptr(tab1)))
                wkeep += [du, am_d]
                dg1, db1 = torch.empty(c, **f32), torch.empty(c, **f32)
                am_g = torch.empty(AMAX_SLOTS, **f32)
                dt1 = torch.empty((rows, c), **f32)
                _lib.check(lib.nw_conv2d_nhwc_f16x2(_ptr(du), am_d.data_ptr() + 4 * AMAX_SLOTS, _ptr(d1.split), _ptr(d1.scale), None,
                                                    None, 0, _ptr(dt1), am_d.data_ptr() + 8 * AMAX_SLOTS, n, h, w, mid, c, 1, 1, 1, 0,
                                                    0, 0, None, st), "nw_conv2d_nhwc_f16x2")
                # norm1 + relu over the slab's prefix: dx is ADDED into the gradient slab's prefix, in place
                _lib.check(lib.nw_bn_relu_nhwc_train_bwd_f32(_ptr(slab), ctot, _ptr(dt1), _ptr(g1), _ptr(b1), _ptr(m1), _ptr(i1),
                                                             _ptr(G), _ptr(dg1), _ptr(db1), _ptr(G), ctot, ctot, _ptr(am_g),
                                                             _ptr(wsn), bnb, rows, c, 1, st), "nw_bn_relu_nhwc_train_bwd_f32")
                grads[6 * k:6 * k + 6] = [dg1, db1, dw1, dg2, db2, dw2]
            if wjobs:
                jobs = (_lib.WgradJob * len(wjobs))(*wjobs)
                wsb = lib.nw_conv2d_nhwc_wgrad_batch_workspace_bytes(jobs, len(wjobs))
                ws = _workspace(wsb, dev)
                _lib.check(lib.nw_conv2d_nhwc_wgrad_batch_f16x2(jobs, len(wjobs), _ptr(ws), wsb, st),
                           "nw_conv2d_nhwc_wgrad_batch_f16x2")
        del wkeep
        dx = None
        if ctx.needs_input_grad[0]:
            dx = G[:, :c0]                  # a channel prefix of the gradient slab (the pools' backward reads strided rows)
            dx.nw_amax = am_g
        return (dx, None, None, *grads)


@torch.no_grad()
def bn_relu_nhwc_apply(x, mean, invstd, gamma, beta, relu=True):
    """relu((x - mean) gamma invstd + beta) over a channels-last fp32 activation with GIVEN statistics (an eval-mode BatchNorm2d
    + ReLU that no convolution follows: DenseNet's norm5) in nw_bn_relu_nhwc_apply_f32; (n, c, h, w), c % 4 == 0."""
    _need_hip(x)
    lib = _lib.load()
    xv, ldx = _nhwc_rows(x)
    n, c, h, w = xv.shape
    y = torch.empty((n, c, h, w), dtype=torch.float32, device=xv.device, memory_format=torch.channels_last)
    amax = torch.empty(AMAX_SLOTS, dtype=torch.float32, device=xv.device)
    with _OnDevice(xv.device):
        _lib.check(lib.nw_bn_relu_nhwc_apply_f32(_ptr(xv), ldx, _ptr(mean), _ptr(invstd), None, _ptr(gamma), _ptr(beta), None, None, None,
                                                 0.0, _ptr(y), _ptr(amax), n * h * w, c, int(relu), _stream(xv)), "nw_bn_relu_nhwc_apply_f32")
    y.nw_amax = amax
    return y


@torch.no_grad()
def bn_relu_avgpool2_nhwc(x, tab):
    """avgpool2x2(relu((x - mean) a + beta)) over a channels-last fp32 activation (tab = bn_table(bn)): an eval-mode DenseNet
    transition's norm -> relu with the pool pulled in front of the 1 x 1 convolution (nw_bn_relu_avgpool2x2_nhwc_f32)."""
    _need_hip(x, tab)
    lib = _lib.load()
    xv, ldx = _nhwc_rows(x)
    n, c, h, w = xv.shape
    y = torch.empty((n, c, h // 2, w // 2), dtype=torch.float32, device=xv.device, memory_format=torch.channels_last)
    amax = torch.empty(AMAX_SLOTS, dtype=torch.float32, device=xv.device)
    with _OnDevice(xv.device):
        _lib.check(lib.nw_bn_relu_avgpool2x2_nhwc_f32(_ptr(xv), ldx, _ptr(tab), _ptr(y), 0, _ptr(amax), n, h, w, c, _stream(xv)),
                   "nw_bn_relu_avgpool2x2_nhwc_f32")
    y.nw_amax = amax
    return y


def bn_table(bn):
    """mean | a | beta (3 c floats) of an eval-mode BatchNorm2d for nw_conv2d_nhwc_bnrelu_f16x2: y = (x - mean) a + beta."""
    from .model.backbones import _bn_scale
    return torch.cat((bn.running_mean.detach().float(), _bn_scale(bn, f32=True), bn.bias.detach().float())).contiguous()


@torch.no_grad()
def dense_block_nhwc_infer(x, plan):
    """A dense block (model/densenet.py:62-80) at inference over ONE channels-last slab, two launches per layer:
    conv1 = nw_conv2d_nhwc_bnrelu_f16x2 (norm1 + relu1 in its loaders, norm2 folded into its weight and bias, relu2 in its
    store) and conv2 = nw_conv2d_nhwc_f16x2 writing its `growth` channels into the slab.  plan: per layer (table of norm1,
    SplitConvWeight of the folded conv1, its bias, SplitConvWeight of conv2).  The bound conv1's loaders need is derived in the
    kernel from the amax records of everything in the slab so far (the input's and every conv2's: `raw_records`).  Returns the
    slab (n, C0 + L growth, h, w) with `.nw_records` (L + 1 records)."""
    lib = _lib.load()
    xv, ldx0 = _nhwc_rows(x)
    n, c0, h, w = xv.shape
    dev, L = xv.device, len(plan)
    growth, mid = plan[0][3].shape[0], plan[0][1].shape[0]
    ctot = c0 + L * growth
    slab = getattr(x, "nw_slab", None)
    if not (slab is not None and tuple(slab.shape) == (n, ctot, h, w) and slab.data_ptr() == xv.data_ptr() and ldx0 == ctot
            and slab.dtype == torch.float32 and slab.is_contiguous(memory_format=torch.channels_last)):
        slab = torch.empty((n, ctot, h, w), dtype=torch.float32, device=dev, memory_format=torch.channels_last)
        slab[:, :c0] = xv
    f32 = dict(dtype=torch.float32, device=dev)
    recs = torch.empty((L + 1) * AMAX_SLOTS, **f32)
    am0 = getattr(x, "nw_amax", None)
    recs[:AMAX_SLOTS].copy_(am0 if am0 is not None else absmax(xv if ldx0 == c0 else xv.contiguous(memory_format=torch.channels_last)))
    u = torch.empty((n * h * w, mid), **f32)
    am_u = torch.empty(AMAX_SLOTS, **f32)
    st = _stream(xv)
    with _OnDevice(dev):
        for k, (tab1, w1, b1, w2) in enumerate(plan):
            c = c0 + k * growth
            kh = w2.shape[2]
            _lib.check(lib.nw_conv2d_nhwc_bnrelu_f16x2(_ptr(slab), _ptr(tab1), _ptr(recs), k + 1, _ptr(w1.split), _ptr(w1.scale), _ptr(b1),
                                                       1, _ptr(u), _ptr(am_u), n, h, w, c, mid, 1, 1, 1, 0, ctot, 0, None, st),
                       "nw_conv2d_nhwc_bnrelu_f16x2")
            _lib.check(lib.nw_conv2d_nhwc_f16x2(_ptr(u), _ptr(am_u), _ptr(w2.split), _ptr(w2.scale), None, None, 0,
                                                slab.data_ptr() + 4 * c, recs.data_ptr() + 4 * AMAX_SLOTS * (k + 1), n, h, w, mid, growth,
                                                kh, kh, 1, kh // 2, 0, ctot, None, st), "nw_conv2d_nhwc_f16x2")
    slab.nw_records = recs
    return slab


@torch.no_grad()
def conv1x1_bnrelu_nhwc_infer(x, tab, weight, records=None, room=0):
    """conv1x1(relu(bn(x))) of a DenseNet transition at inference (model/densenet.py:86-90; nw_conv2d_nhwc_bnrelu_f16x2)
    over a channels-last activation; records: the amax records of x's producers (default: x.nw_records / x.nw_amax)."""
    lib = _lib.load()
    xv, ldx = _nhwc_rows(x)
    n, c, h, w = xv.shape
    cout = weight.shape[0]
    if records is None:
        records = getattr(x, "nw_records", None)
        if records is None:
            records = getattr(x, "nw_amax", None)
        if records is None:
            records = absmax(xv if ldx == c else xv.contiguous(memory_format=torch.channels_last))
    y, ldy = _with_room(n, cout, h, w, room, xv.device)
    am = torch.empty(AMAX_SLOTS, dtype=torch.float32, device=xv.device)
    with _OnDevice(xv.device):
        _lib.check(lib.nw_conv2d_nhwc_bnrelu_f16x2(_ptr(xv), _ptr(tab), _ptr(records), records.numel() // AMAX_SLOTS, _ptr(weight.split),
                                                   _ptr(weight.scale), None, 0, _ptr(y), _ptr(am), n, h, w, c, cout, 1, 1, 1, 0, ldx,
                                                   ldy if room > 0 else 0, None, _stream(xv)), "nw_conv2d_nhwc_bnrelu_f16x2")
    y.nw_amax = am
    return y


def dense_block_nhwc_supported(x, layers, bank):
    """Can ops.dense_block_nhwc_train run this block?  (channels-last fp32 on the device, a weight bank that holds every
    layer's forward and data-gradient operands, affine BatchNorms, no dropout, shapes the convolution kernels serve)"""
    if bank is None or not x.is_cuda or x.dim() != 4 or not layers:
        return False
    lib = _lib.load()
    n, c0, h, w = x.shape
    growth, mid = layers[0].conv2.weight.shape[0], layers[0].conv1.weight.shape[0]
    if n * h * w <= 1 or c0 % 32 or growth % 32 or mid % 32 or c0 + len(layers) * growth > BN_NHWC_MAX_C:
        return False
    for k, layer in enumerate(layers):
        c = c0 + k * growth
        w1, w2 = layer.conv1.weight, layer.conv2.weight
        kh = w2.shape[2]
        if (layer.drop_rate > 0 or tuple(w1.shape) != (mid, c, 1, 1) or tuple(w2.shape) != (growth, mid, kh, kh) or kh % 2 == 0
                or not (layer.norm1.affine and layer.norm2.affine) or layer.norm1.weight is None or layer.norm2.weight is None
                or layer.norm1.eps != layers[0].norm1.eps or layer.norm2.eps != layers[0].norm1.eps):
            return False
        for wt in (w1, w2):
            ops_ = bank.operands(wt) if bank.has(wt) else None
            if ops_ is None or ops_[0] is None or ops_[1] is None:
                return False
        if not (lib.nw_conv2d_nhwc_wgrad_supported(n, h, w, c, mid, 1, 1, 1, 0)
                and lib.nw_conv2d_nhwc_wgrad_supported(n, h, w, mid, growth, kh, kh, 1, kh // 2)):
            return False
    return True


def dense_block_nhwc_train(x, layers, bank):
    """The dense block `layers` (modules with norm1, conv1, norm2, conv2) over a channels-last activation as one autograd node
    over one slab (_DenseBlockNhwcFn); returns the block's output (n, C0 + L growth, h, w), channels_last."""
    params = []
    for layer in layers:
        params += [layer.norm1.weight, layer.norm1.bias, layer.conv1.weight, layer.norm2.weight, layer.norm2.bias,
                   layer.conv2.weight]
    _need_hip(x, *params)
    return _DenseBlockNhwcFn.apply(x, tuple(layers), bank, *params)


def conv2d_nhwc_train(x, weight, stride=1, pad=0, amax=None, operands=None, room=0):
    """Differentiable conv2d(x, weight, stride=stride, padding=pad) for channels-last fp32 activations on the MI355X
    (bias-free: the backbones' convolutions have none).  x may carry `.nw_amax`; operands: ConvWeightBank.operands(weight)
    (else the weight is split inside the call, forward and backward)."""
    _need_hip(x, weight)
    return _ConvNhwcFn.apply(x, weight, int(stride), int(pad), amax, operands, int(room))
