"""Records what the head entry points of nwhead_amd.ops hand to the C library (a plain helper module, like ws_poison.py).

ops.nw_head, nw_partials(_into), nw_scores, nw_knn, nw_head_influence and ShardedBank decide per call which rows, labels,
norms, operand tensors, query width and nw_fwd_opts the library receives (ops.SplitBank's docstring has the rules).  The
Recorder swaps ``ops._lib.load`` for a proxy that forwards every call and notes, for the forward entry points, the scalars,
the ROLE of every pointer (found by address among the tensors the case knows) and the decoded options.  case_ids() is the table
of (bank, call) pairs over the smallest shapes at which each rule can go wrong; tests/golden/record_bank_calls.py writes
its records from the parent of a change, tests/test_bank_calls_gpu.py requires the code under test to reproduce them.
"""
import ctypes

import torch

B, C = 3, 5

# entry -> argument names in the order of include/nwhead_hip.h ("stream" is skipped, "opts" decoded, "ws_bytes" kept apart)
ENTRIES = {
    "nw_fwd_f32": "q s sy norm2 operand scale out scores lse weights ws ws_bytes B N d C kind ls sup_batched lab_batched opts stream",
    "nw_fwd_partial_f32": "q s sy norm2 operand scale m den num ws ws_bytes B N d C kind ls opts stream",
    "nw_fwd_influence_f32": "q s sy norm2 operand scale qy out lse infl ws ws_bytes B N d C kind ls opts stream",
    "nw_knn_f32": "q operand scale norm2 idx vals ws ws_bytes B N d k kind ls stream",
    "nw_scores_f32": "q s out B N d kind ls batched stream",
    "nw_split_rows_f16x2": "s operand scale norm2 N d stream",
}
ENTRIES = {k: v.split() for k, v in ENTRIES.items()}
BANK_ROLES = ("rows", "sorted_rows", "sorted_labels", "split", "scale", "norm2", "packed", "packed_scale", "packed_norm2")


class Recorder:
    """``with Recorder(ops, q=q, s=s, labels=sy, bank=bank) as rec: ...; rec.calls`` -- the records of the calls made inside."""

    def __init__(self, ops, q=None, s=None, labels=None, bank=None, entries=ENTRIES):
        self.ops, self.bank, self.calls, self.entries = ops, bank, [], entries
        self.roles = {}
        for role, t in (("q", q), ("s", s), ("labels", labels)):
            if t is not None:
                self.roles.setdefault(t.data_ptr(), role)
        for name in BANK_ROLES if bank is not None else ():
            t = getattr(bank, name)
            if t is not None:
                self.roles.setdefault(t.data_ptr(), "bank." + name)

    def __enter__(self):
        from nwhead_amd import _lib
        self._lib_mod, self._load = _lib, self.ops._lib.load
        real, rec, entries = self._load(), self, self.entries

        class Proxy:
            def __getattr__(self, name):
                fn = getattr(real, name)
                if name not in entries:
                    return fn
                return lambda *a: (rec._note(name, a), fn(*a))[1]

        proxy = Proxy()
        self.ops._lib.load = lambda: proxy
        return self

    def __exit__(self, *exc):
        self.ops._lib.load = self._load

    def _role(self, addr):
        return None if not addr else self.roles.get(addr, "other")

    def _note(self, entry, args):
        names = self.entries[entry]
        assert len(args) == len(names), (entry, len(args))
        sig = self._lib_mod.SIGNATURES[entry][1]
        a = dict(zip(names, args))
        r = {"entry": entry, "scalars": {}, "pointers": {}, "workspace_bytes": a.get("ws_bytes")}
        for name, typ, v in zip(names, sig, args):
            if name in ("stream", "ws_bytes", "opts"):
                continue
            if typ is ctypes.c_void_p:
                r["pointers"][name] = self._role(v)
            else:
                r["scalars"][name] = int(v)
        if "opts" in a:
            o = self._lib_mod.FwdOpts.from_address(a["opts"])
            tables = self.bank.tables if self.bank is not None else None
            r["opts"] = {"persistent_wgs": o.persistent_wgs, "force_split": o.force_split, "operand_form": o.operand_form,
                         "tables": None if not o.tables else ("bank.tables" if tables is not None and o.tables == tables.data_ptr()
                                                              else "other"),
                         "tables_N": o.tables_N, "tables_sy_is_labels": bool(o.tables_sy) and o.tables_sy == a.get("sy")}
        self.calls.append(r)


# ---- the case table
def _labels(N, order, g):
    sy = (torch.arange(N) % C).sort().values
    return sy[torch.randperm(N, generator=g)] if order == "shuffled" else sy


# name -> (precision or None for "no bank", d, N, labels the bank is built with: "sorted" | "shuffled" | None)
BANKS = {
    "f32_sorted": ("fp32", 64, 40, "sorted"),
    "f32_nolabels": ("fp32", 64, 40, None),
    "f32_shuffled": ("fp32", 64, 40, "shuffled"),
    "f32_d72_sorted": ("fp32", 72, 40, "sorted"),           # pads to 96
    "f32_d72_shuffled": ("fp32", 72, 40, "shuffled"),
    "f32_d40": ("fp32", 40, 40, "sorted"),                  # norms only
    "f32_d42": ("fp32", 42, 40, "sorted"),                  # norms only and d % 4
    "f32_N42": ("fp32", 64, 42, "sorted"),                  # N % 4 != 0
    "f16_sorted": ("fp16", 192, 40, "sorted"),
    "f16_d100_shuffled": ("fp16", 100, 40, "shuffled"),     # pads to 192
    "f16_N20": ("fp16", 192, 20, "sorted"),                 # norms only
    "none_d64": (None, 64, 40, "sorted"),
    "none_d66": (None, 66, 40, "sorted"),
}
HEAD_CALLS = ("head", "head_weights", "head_int32", "head_copy", "head_qgrad", "head_sgrad")
BANK_CALLS = HEAD_CALLS + ("partials", "partials_into_wgs8", "scores", "knn5", "knn33", "knn5_nosupport", "influence",
                           "sharded_predict", "sharded_partial")
NOBANK_CALLS = HEAD_CALLS + ("head_batched", "partials", "influence", "scores")


def train_shape(lib):
    """The smallest (B, N) at which a training step of width 257 (-> 260 by the d % 4 rule -> 288 by the d % 32 rule) has its
    backward on split rows, as nw_bwd_uses_split answers."""
    cands = sorted(((b, n) for b in (8, 16, 32, 64, 128) for n in (128, 256, 512, 1024)), key=lambda t: (t[0] * t[1], t[1]))
    return next((b, n) for b, n in cands if lib.nw_bwd_uses_split(b, n, 288, C, 0))


def case_ids():
    ids = []
    for bank, (prec, d, N, order) in BANKS.items():
        if prec is None:
            ids += [f"{bank}/{c}{n2}" for c in NOBANK_CALLS for n2 in ("", "+norm2") if n2 == "" or c in HEAD_CALLS]
            continue
        # (a bank with a class-sorted copy: nw_partials_into is given that copy by hand)
        ids += [f"{bank}/{'partials_into_by_hand' if c == 'partials_into_wgs8' and order == 'shuffled' else c}" for c in BANK_CALLS]
    return ids + ["none_d257/train_step"]


_INPUTS = {}


def _inputs(ops, dev, bank_name):
    """Seeded (q, s, sy, bank) of one bank of the table, built once."""
    got = _INPUTS.get((bank_name, str(dev)))
    if got is None:
        prec, d, N, order = BANKS[bank_name]
        g = torch.Generator().manual_seed(1000 * d + N)
        q, s = torch.randn(B, d, generator=g).to(dev), torch.randn(N, d, generator=g).to(dev)
        sy = _labels(N, order or "sorted", g).to(dev)
        bank = None if prec is None else ops.SplitBank(s, labels=sy if order else None, precision=prec)
        got = _INPUTS[(bank_name, str(dev))] = (q, s, sy, bank)
    return got


def _tensors(out):
    out = out if isinstance(out, (tuple, list)) else (out,)
    return [t.detach().clone() for t in out]


def run_case(ops, dev, case_id):
    """-> (records, output tensors, "Type: message" of the exception the call raised or None) of one case.  The cached
    workspaces are dropped first, so that the buffer a call finds (and the size it names) does not depend on earlier calls."""
    from nwhead_amd.sharded import ShardedBank
    bank_name, call = case_id.split("/")
    ops._WS_CACHE.clear()
    if call == "train_step":
        Bt, Nt = train_shape(ops._lib.load())
        g = torch.Generator().manual_seed(257)
        q = torch.randn(Bt, 257, generator=g).to(dev).requires_grad_()
        s = torch.randn(Nt, 257, generator=g).to(dev).requires_grad_()
        sy = _labels(Nt, "sorted", g).to(dev)
        with Recorder(ops, q=q, s=s, labels=sy) as rec:
            out = ops.nw_head(q, s, sy, C)
        return rec.calls, _tensors(out), None
    q, s, sy, bank = _inputs(ops, dev, bank_name)
    call, _, with_norm2 = call.partition("+")
    kw = {"support_cache": bank} if bank is not None else {}
    if with_norm2:
        kw["support_norm2"] = ops.row_norm2(s)
    if call.startswith("sharded"):
        sb = ShardedBank(s, sy, C, precision=BANKS[bank_name][0])
        bank = sb.cache
    packed = torch.empty(B * (C + 2), dtype=torch.float32, device=dev)
    labels = {"head_int32": sy.to(torch.int32), "head_copy": sy.clone()}.get(call, sy)
    if call == "head_batched":
        s, labels = s.expand(B, -1, -1).contiguous(), sy.expand(B, -1).contiguous()
    if call == "partials_into_by_hand":
        s, labels = bank.sorted_rows, bank.sorted_labels
    if call == "head_qgrad":
        q = q.detach().requires_grad_()          # (same storage: the bank still matches, the roles still resolve)
    if call == "head_sgrad":
        s = s.detach().requires_grad_()
    out, raised = (), None
    with Recorder(ops, q=q, s=s, labels=labels, bank=bank) as rec:
        try:
            if call.startswith("head"):
                out = ops.nw_head(q, s, labels, C, return_weights=call == "head_weights", **kw)
            elif call == "partials":
                out = ops.nw_partials(q, s, labels, C, **kw)
            elif call in ("partials_into_wgs8", "partials_into_by_hand"):
                out = ops.nw_partials_into(packed, q, s, labels, C, cache=bank, persistent_wgs=8)
            elif call == "scores":
                out = ops.nw_scores(q, s, **kw)
            elif call.startswith("knn"):
                out = ops.nw_knn(q, bank, 33 if call == "knn33" else 5, return_values=True,
                                 support=None if call == "knn5_nosupport" else s)
            elif call == "influence":
                out = ops.nw_head_influence(q, s, labels, C, torch.arange(B, device=dev) % C, **kw)
            elif call == "sharded_predict":
                out = sb.predict(q)
            elif call == "sharded_partial":
                sb._hip_partial(packed, q)
                out = packed
            else:
                raise KeyError(case_id)
        except (ValueError, ops.NWHipError) as e:
            raised = f"{type(e).__name__}: {e}"
    return rec.calls, _tensors(out), raised
