"""The neighbour-search callers' routes, case by case (a plain helper module, next to bank_call_recorder.py).

ops.nw_knn, KNN.indices, NWNet.get_neighbors and ShardedBank decide per search between the fp16-rounded search
(nw_knn_f16), the fused split-row search (nw_knn_f32 / nw_knn_window_f32) and a score matrix ranked by nw_topk_f32 or
torch (ops.knn_route has the rule).  run_case() runs one case through the PUBLIC callers only -- so that it runs on the
parent of a change as well -- under bank_call_recorder's Recorder with the search entries added to its table, and returns
the library calls, the exception and the result (rows, and the bit patterns of values).
tests/golden/record_knn_calls.py writes the records from the parent of a change, tests/test_knn_calls_gpu.py requires the
code under test to reproduce them.
"""
import os

import torch

import bank_call_recorder as R

B, C = R.B, R.C

ENTRIES = dict(R.ENTRIES)
ENTRIES.update({k: v.split() for k, v in {
    "nw_knn_window_f32": "q operand scale norm2 row_lo row_hi exclude idx vals ws ws_bytes B N d k kind ls stream",
    "nw_knn_f16": "q operand scale norm2 idx vals ws ws_bytes B N d k kind ls opts stream",
    "nw_topk_f32": "scores idx vals B N k stream",
    "nw_knn_workspace_bytes": "B N d k",
    "nw_knn_f16_workspace_bytes": "B N d k",
}.items()})

BANKS = {name: R.BANKS[name] for name in ("f32_sorted", "f32_nolabels", "f32_shuffled", "f32_N42", "f32_d40", "f16_sorted",
                                          "f16_d100_shuffled", "f16_N20")}
BANKS["f16_shuffled"] = ("fp16", 192, 40, "shuffled")

KNN_CALLS = ("knn5", "knn33", "knn5_nosupport", "knn5_rounded", "knn5_window", "knn5_window_excluded", "knn5_rounded_window")
# <caller>-<search_precision>-<gate>: gate "open" patches ops.KNN_FUSED_MIN_SCORE_BYTES to 0, "closed" leaves its default
GATED = tuple(f"{c}-{sp}-{gate}" for c in ("indices", "neighbors") for sp in ("fp32", "fp16") for gate in ("closed", "open"))
SHARDED = tuple(f"{c}-{sp}" for c in ("sharded_neighbors", "sharded_predict_knn") for sp in ("fp32", "fp16"))
CALLS = KNN_CALLS + GATED + ("neighbors_all-fp32-open",) + SHARDED


def case_ids():
    # (the suite pins NW_SPLIT_ALWAYS=1; without it a search of this size ranks the score matrix by the size rule)
    return [f"{bank}/{call}" for bank in BANKS for call in CALLS] + ["f32_nolabels/knn5_size_rule"]


_INPUTS = {}


def _inputs(ops, dev, bank_name):
    """Seeded (q, s, sy, bank) of one bank of the table, built once (bank_call_recorder._inputs over this table)."""
    got = _INPUTS.get((bank_name, str(dev)))
    if got is None:
        prec, d, N, order = BANKS[bank_name]
        g = torch.Generator().manual_seed(1000 * d + N)
        q, s = torch.randn(B, d, generator=g).to(dev), torch.randn(N, d, generator=g).to(dev)
        sy = R._labels(N, order or "sorted", g).to(dev)
        got = _INPUTS[(bank_name, str(dev))] = (q, s, sy, ops.SplitBank(s, labels=sy if order else None, precision=prec))
    return got


def encode(out):
    """Result tensors as JSON: integer tensors by value, floating ones by bit pattern."""
    out = out if isinstance(out, (tuple, list)) else (out,)
    return [{"dtype": str(t.dtype), "shape": list(t.shape),
             "data": (t.contiguous().view(torch.int32) if t.is_floating_point() else t).flatten().tolist()} for t in out]


def run_case(ops, dev, case_id):
    """-> {"calls": the library calls, "raises": "Type: message" or None, "out": encode(result)} of one case.  Cached
    workspaces and workspace sizes are dropped first, so that what a call asks and finds does not depend on earlier ones."""
    from nwhead_amd.nwhead.nw import NWNet
    from nwhead_amd.nwhead.utils import KNN
    from nwhead_amd.sharded import ShardedBank
    bank_name, call = case_id.split("/")
    q, s, sy, bank = _inputs(ops, dev, bank_name)
    prec, N = BANKS[bank_name][0], BANKS[bank_name][2]
    ops._WS_CACHE.clear()
    ops._WS_BYTES.clear()
    # windows of bank rows, one per query: a few rows, the empty window, all rows but the first
    lo = torch.tensor([2, 7, 1], dtype=torch.int32, device=dev)
    hi = torch.tensor([9, 7, N], dtype=torch.int32, device=dev)
    name, _, rest = call.partition("-")
    sp, _, gate = rest.partition("-")
    gate_bytes, env = ops.KNN_FUSED_MIN_SCORE_BYTES, os.environ.get("NW_SPLIT_ALWAYS")
    out, raised = (), None
    with R.Recorder(ops, q=q, s=s, labels=sy, bank=bank, entries=ENTRIES) as rec:
        rec.roles.update({lo.data_ptr(): "row_lo", hi.data_ptr(): "row_hi"})
        try:
            if gate == "open":
                ops.KNN_FUSED_MIN_SCORE_BYTES = 0
            if name == "knn5_size_rule":
                os.environ.pop("NW_SPLIT_ALWAYS", None)
            if name.startswith("knn"):
                kw = {"support": None if name == "knn5_nosupport" else s, "rounded": "rounded" in name}
                if "window" in name:
                    kw.update(row_window=(lo, hi), exclude=name.endswith("excluded"))
                out = ops.nw_knn(q, bank, 33 if name == "knn33" else 5, return_values=True, **kw)
            elif name == "indices":
                knn = KNN(s, sy, n_neighbors=5, search_precision=sp)
                knn.bank = bank
                out = knn.indices(q)
            elif name.startswith("neighbors"):
                net = NWNet(torch.nn.Identity(), C, full_precision=prec, search_precision=sp)
                net.full_feat, net.full_y, net.full_cache = s, sy, bank     # what precompute() leaves
                out = net.get_neighbors(q, None if name == "neighbors_all" else 5)
            elif name.startswith("sharded"):
                sb = ShardedBank(s, sy, C, precision=prec, search_precision=sp, persistent_wgs=8)
                shard = {role: getattr(sb.cache, role) for role in R.BANK_ROLES}
                rec.roles.update({t.data_ptr(): "shard." + role for role, t in shard.items() if t is not None})
                out = sb.predict_knn(q, 5) if name == "sharded_predict_knn" else sb.neighbors(q, 5, True, True)
            else:
                raise KeyError(case_id)
        except (ValueError, ops.NWHipError) as e:
            raised = f"{type(e).__name__}: {e}"
        finally:
            ops.KNN_FUSED_MIN_SCORE_BYTES = gate_bytes
            if env is not None:
                os.environ["NW_SPLIT_ALWAYS"] = env
    return {"calls": rec.calls, "raises": raised, "out": encode(out)}
