"""The callers of the head over a resident bank, case by case (a plain helper module, next to knn_call_recorder.py).

ops.nw_head(row_window=... / row_logw=...), ops.nw_head_window and ops.nw_head_bank decide per call between the fused
entries (nw_fwd_window_f32, nw_fwd_weighted_f32; nw_bwd_query_f32, nw_bwd_query_weighted_f32, nw_bwd_query_logw_f32 with
their workspace-size calls), the route through the score matrix (nw_scores_f32, a torch mask, nw_aggregate_f32), nw_head's
own route (nw_fwd_f32, nw_bwd_bank_f32) and a refusal (ops.head_bank_refusal has the rule).  run_case() runs one case
through the PUBLIC callers only -- so that it runs on the parent of a change as well -- under bank_call_recorder's Recorder
with these entries in its table, and returns the library calls, the exception and the bits of the results and gradients.
tests/golden/record_bank_head_calls.py writes the records from the parent of a change, tests/test_bank_head_calls_gpu.py
requires the code under test to reproduce them.
"""
import math

import torch

import bank_call_recorder as R
from knn_call_recorder import encode

C = R.C

_HEAD = "q operand scale norm2 sy"
_TAIL = "ws ws_bytes B N d C kind ls"
ENTRIES = dict(R.ENTRIES)
ENTRIES.update({k: v.split() for k, v in {
    "nw_fwd_window_f32": f"{_HEAD} row_lo row_hi exclude out lse {_TAIL} stream",
    "nw_fwd_weighted_f32": f"{_HEAD} row_logw row_lo row_hi exclude out lse {_TAIL} stream",
    "nw_bwd_query_f32": f"{_HEAD} row_lo row_hi exclude lse out gout gq gls {_TAIL} row_chunks stream",
    "nw_bwd_query_weighted_f32": f"{_HEAD} row_logw row_lo row_hi exclude lse out gout gq gls {_TAIL} row_chunks stream",
    "nw_bwd_query_logw_f32": f"{_HEAD} row_logw row_lo row_hi exclude lse out gout gq glogw gls {_TAIL} row_chunks stream",
    "nw_bwd_query_workspace_bytes": "B N d C row_chunks",
    "nw_bwd_logw_workspace_bytes": "B N d C row_chunks want_gq",
    "nw_aggregate_f32": "scores sy out lse weights B N C lab_batched stream",
    "nw_bwd_bank_f32": f"q s norm2 operand scale sy scores lse out gout gq gs gls {_TAIL} sup_batched lab_batched stream",
    "nw_bwd_workspace_bytes": "B N d C kind sup_batched",
}.items()})

# name -> (precision, d, N, labels the bank is built with): the smallest shapes at which a rule can go wrong
BANKS = {
    "d64_N40": ("fp32", 64, 40, "sorted"),                # the fused route
    "d72_N40": ("fp32", 72, 40, "sorted"),                # the bank pads to 96, and the queries with it
    "d64_N26": ("fp32", 64, 26, "sorted"),                # the smallest bank the kernels take
    "d64_N25": ("fp32", 64, 25, "sorted"),                # below the kernels: the matrix route or a refusal
    "d64_N130": ("fp32", 64, 130, "sorted"),              # three 64-row support tiles
    "d64_N40_shuffled": ("fp32", 64, 40, "shuffled"),     # a class-sorted copy: the matrix route or a refusal
    "f16_d192_N40": ("fp16", 192, 40, "sorted"),          # no split rows: the matrix route or a refusal
}
# <caller>_<window>_<weights>[_<what requires grad>]; windows: kept [5, 20), loo = [i, i+1) excluded, empty = kept with one
# query at lo >= hi, dead = kept [3, 4) and [10, 11) for two queries, rows whose weight is -inf.  grad: q, a (the weights),
# qa, ls (the clip scale alone), none; qgrad / short: nw_head refuses a query gradient / weights of the wrong length
INFERENCE = ("head_kept_none", "head_loo_none", "head_empty_none", "head_none_w", "head_kept_w", "head_loo_w", "head_dead_w",
             "window_kept_none_lse", "window_loo_w_lse", "head_kept_none_qgrad", "head_none_w_short")
GRADIENTS = ("bank_none_none_q", "bank_kept_none_q", "bank_loo_none_q", "bank_none_w_q", "bank_loo_w_q", "bank_none_w_qa",
             "bank_kept_w_qa", "bank_none_w_a", "bank_dead_w_a", "bank_none_none_none", "bank_kept_w_none")
CALLS = INFERENCE + GRADIENTS
# on the N = 40 bank: clip with a logit_scale (one case asks for the scale's gradient alone, one for it beside q's), and
# B = 70 -- two 64-query tiles, the weights' gradient summed over query tiles -- with and without gq
EXTRA = {"d64_N40": ("head_kept_w+clip", "bank_loo_none_q+clip", "bank_none_w_qa+clip", "bank_kept_w_ls+clip",
                     "bank_none_none_ls+clip", "bank_kept_w_qa+B70", "bank_kept_w_a+B70")}
PATTERN = (0.0, math.log(2.0), -3.5, float("-inf"), 0.0, 1.25, -0.5)      # of tools/weighted_time.py, by j mod 7


def case_ids(bank=None):
    return [f"{b}/{c}" for b in BANKS if bank in (None, b) for c in CALLS + EXTRA.get(b, ())]


class _Recorder(R.Recorder):
    """Recorder that keeps the address of a pointer it cannot name yet: the gradients exist only once the backward has run."""

    def _role(self, addr):
        return None if not addr else self.roles.get(addr, addr)

    def resolve(self, grads):
        """``grads``: argument name -> the tensor that holds that gradient now, or None.  Only the argument of that name can
        be it (an address seen earlier may have been freed and handed out again since)."""
        for r in self.calls:
            r["pointers"] = {k: v if not isinstance(v, int) else k if grads.get(k) is not None and grads[k].data_ptr() == v
                             else "other" for k, v in r["pointers"].items()}
        return self.calls


_INPUTS = {}


def _inputs(ops, dev, bank_name, B):
    """Seeded (q, s, sy, bank) of one bank of the table and one batch size, built once."""
    got = _INPUTS.get((bank_name, B, str(dev)))
    if got is None:
        prec, d, N, order = BANKS[bank_name]
        g = torch.Generator().manual_seed(1000 * d + N)
        q, s = torch.randn(70, d, generator=g)[:B].contiguous().to(dev), torch.randn(N, d, generator=g).to(dev)
        sy = R._labels(N, order, g).to(dev)
        got = _INPUTS[(bank_name, B, str(dev))] = (q, s, sy, ops.SplitBank(s, labels=sy, precision=prec))
    return got


def _window(kind, B, N, dev):
    i = torch.arange(B, dtype=torch.int32) % N
    if kind == "none":
        return None, False
    if kind == "loo":
        lo, hi = i, i + 1
    elif kind == "dead":                  # rows 3 and 10 have the weight -inf: queries 0 and 1 admit nothing else
        lo = torch.full((B,), 5, dtype=torch.int32)
        lo[0], lo[1] = 3, 10
        hi = torch.where(lo == 5, torch.full_like(lo, 20), lo + 1)
    else:
        lo, hi = torch.full((B,), 5, dtype=torch.int32), torch.full((B,), 20, dtype=torch.int32)
        if kind == "empty":
            lo[1], hi[1] = 9, 9
    return (lo.to(dev), hi.to(dev)), kind == "loo"


def run_case(ops, dev, case_id):
    """-> {"calls": the library calls, "raises": "Type: message" or None, "out": encode(results and gradients)} of one case.
    Cached workspaces and workspace sizes are dropped first, so that what a call asks and finds does not depend on earlier
    ones."""
    bank_name, call = case_id.split("/")
    call, _, variant = call.partition("+")
    caller, win, wts, *rest = call.split("_")
    what = rest[0] if rest else ""
    B = 70 if variant == "B70" else R.B
    q, s, sy, bank = _inputs(ops, dev, bank_name, B)
    N = s.shape[0]
    ops._WS_CACHE.clear()
    ops._WS_BYTES.clear()
    window, exclude = _window(win, B, N, dev)
    a = torch.tensor(PATTERN)[torch.arange(N) % 7].to(dev) if wts == "w" else None
    kind, ls = "euclidean", None
    if variant == "clip":
        kind, ls = "clip", torch.tensor(1.75, device=dev)
    grad = what if caller == "bank" else "q" if what == "qgrad" else ""
    if "q" in grad:
        q = q.detach().requires_grad_()          # (same storage: the roles still resolve)
    if "a" in grad:
        a = a.requires_grad_()
    if grad == "ls" or (ls is not None and "q" in grad):
        ls = ls.requires_grad_()
    if what == "short":
        a = torch.zeros(N - 1, device=dev)
    out, raised = (), None
    with _Recorder(ops, q=q, s=s, labels=sy, bank=bank, entries=ENTRIES) as rec:
        if window is not None:
            rec.roles.update({window[0].data_ptr(): "row_lo", window[1].data_ptr(): "row_hi"})
        if a is not None:
            rec.roles[a.data_ptr()] = "row_logw"
        try:
            if caller == "head":
                out = ops.nw_head(q, s, sy, C, kind, ls, support_cache=bank, row_window=window, exclude=exclude, row_logw=a)
            elif caller == "window":
                out = ops.nw_head_window(q, s, sy, C, bank, window, exclude, kind, ls, return_lse=True, row_logw=a)
            elif caller == "bank":
                out = ops.nw_head_bank(q, s, sy, C, bank, kind, ls, row_window=window, exclude=exclude, row_logw=a)
                if out.requires_grad:
                    g = torch.Generator().manual_seed(B)
                    out.backward(torch.randn(B, C, generator=g).to(dev))
            else:
                raise KeyError(case_id)
        except (ValueError, ops.NWHipError) as e:
            raised = f"{type(e).__name__}: {e}"
        grads = {"gq": q.grad, "glogw": None if a is None else a.grad, "gls": None if ls is None else ls.grad}
        calls = rec.resolve(grads)
    out = list(out) if isinstance(out, (tuple, list)) else [out]
    # (the results, then q.grad, row_logw.grad and logit_scale.grad where there is one)
    return {"calls": calls, "raises": raised, "out": encode([t.detach() for t in out + [t for t in grads.values() if t is not None]])}
