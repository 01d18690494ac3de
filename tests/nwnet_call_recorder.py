"""The public entry points of NWNet over its banks, case by case (a plain helper module, next to bank_head_call_recorder.py).

NWNet decides per call which bank serves it -- precompute()'s resident one, precompute_sharded()'s shards, what
support_eval builds per call -- or refuses (nw.bank_rule has the rule), rebuilds the resident bank's SplitBank or not, and
hands ops.nw_head / nw_head_bank / nw_knn / nw_top_influence / SplitBank.update_rows their operands.  run_case() builds a
real NWNet over a toy dataset whose "images" are the feature rows (the featurizer is the identity), brings it into the bank
state of the case, and runs one call through PUBLIC methods only -- so that it runs on the parent of a change as well --
under bank_head_call_recorder's recorder with the neighbour-search, influence and row-update entries added to its table.
It returns the library calls, the exception, the bits of the results and gradients, and the state the call leaves.
tests/golden/record_nwnet_calls.py writes the records from the parent of a change, tests/test_nwnet_calls_gpu.py requires
the code under test to reproduce them.
"""
import ctypes

import numpy as np
import torch
import torch.nn as nn

import bank_call_recorder as R
import bank_head_call_recorder as H
import knn_call_recorder as K

B, C = R.B, R.C

ENTRIES = dict(H.ENTRIES)
ENTRIES.update(K.ENTRIES)
ENTRIES.update({k: v.split() for k, v in {
    "nw_bank_update_rows_f32": "x rows R dx momentum s_rows s_user s_norm2 s_split s_scale s_f16 f16_scale f16_norm2 N d stream",
    "nw_influence_select_f32": "vals rows sy qy out lse infl_out label_out B k N C stream",
    "nw_pack_rows_f16": "s out scale norm2 N d stream",
    "nw_row_norm2_f32": "x n2 rows d stream",
    "nw_merge_finalize_f32": "m den num out G B C stride_m stride_den stride_num class_lo C_local stream",
    "nw_knn_merge_f32": "vals rows labels G B kc stride_g k C idx_out val_out label_out out stream",
}.items()})

# name -> (full_precision, d, rows per class and environment, environments): the smallest shapes at which a rule can go wrong
NETS = {
    "d64_N40": ("fp32", 64, 8, 1),                 # class-sorted: the fused routes
    "d72_N40": ("fp32", 72, 8, 1),                 # the bank pads to 96, and the queries with it
    "f16_d192_N40": ("fp16", 192, 8, 1),           # no split rows: the matrix route or a refusal; the rounded search
    "d64_N40_2env": ("fp32", 64, 4, 2),            # two environments: labels not class-sorted, the matrix route or a refusal
    "d64_N25": ("fp32", 64, 5, 1),                 # below the kernels
}
STATES = ("resident", "sharded", "both")            # precompute() | precompute_sharded() | precompute(), then precompute_sharded()
# <entry>[-<argument>][+<option>]...; options: w / lw constant / learnable support weights, leave_out, bwd, open (the size gate
# of the fused search open: ops.KNN_FUSED_MIN_SCORE_BYTES = 0), sp16 (search_precision="fp16"), per_query, custom (a custom
# kernel module), mask (return_mask=True), stale (full_feat updated in place since precompute())
EVERY_NET = ("precompute", "predict-full", "predict-full+w", "predict-full+leave_out", "predict-full+leave_out+w", "predict_loo",
             "forward_bank+w+bwd", "forward_bank+leave_out+bwd", "refresh_bank-bank_features", "get_neighbors-5",
             "get_neighbors-5+open", "explain-3")
EVERY_STATE = EVERY_NET + (
    "predict-random", "predict-cluster", "predict-ensemble", "predict-knn", "predict-hnsw", "predict-knn+per_query",
    "predict-full+lw", "predict-full+stale", "predict_loo-rows", "predict_loo-rows+w", "forward_bank+bwd", "forward_bank+lw+bwd",
    "refresh_bank-feats", "refresh_bank-nothing", "get_neighbors-None", "get_neighbors-33+open", "get_neighbors-0",
    "get_neighbors-41", "get_neighbors-5+stale", "explain-None", "explain-3+stale", "set_support_weights-short",
    "set_support_weights-nan", "set_support_weights-inf", "set_support_weights-neginf+lw", "set_support_weights-ok",
    "predict-full+custom", "predict-full+leave_out+custom", "get_neighbors-5+custom", "explain-3+custom", "predict_loo+custom",
    "forward_bank+custom", "predict-full+mask", "predict_loo-rows+mask", "forward_bank+mask+bwd", "predict-knn+mask")
HALF = ("get_neighbors-5+sp16", "predict-knn+sp16", "predict-knn+sp16+per_query")


def case_ids(net=None):
    ids = [f"d64_N40/{s}/{c}" for s in STATES for c in EVERY_STATE]
    ids += [f"{n}/resident/{c}" for n in NETS if n != "d64_N40" for c in EVERY_NET]
    ids += [f"f16_d192_N40/{s}/{c}" for s in ("resident", "sharded") for c in HALF]
    return [i for i in ids if net in (None, i.split("/")[0])]


class _Dataset(torch.utils.data.Dataset):
    def __init__(self, data, targets):
        self.data, self.targets = data, list(targets)

    def __len__(self):
        return len(self.targets)

    def __getitem__(self, i):
        return self.data[i], self.targets[i]


class _NegDistance(nn.Module):
    """A custom kernel module, as the reference accepts: torch ops on the device."""

    def forward(self, x, y):
        return -torch.cdist(x, y)


class _Recorder(H._Recorder):
    def _note(self, entry, args):
        super()._note(entry, args)
        for name, typ, v in zip(self.entries[entry], self._lib_mod.SIGNATURES[entry][1], args):
            if typ is ctypes.c_float:
                self.calls[-1]["scalars"][name] = float(v)


def _net(NWNet, net_name, opts):
    prec, d, per, envs = NETS[net_name]
    g = torch.Generator().manual_seed(1000 * d + per * envs)
    targets = [c for _e in range(envs) for c in range(C) for _ in range(per)]
    ds = _Dataset(torch.randn(len(targets), d, generator=g), targets)
    env = None if envs == 1 else np.repeat(np.arange(envs), C * per)
    net = NWNet(nn.Identity(), C, support_dataset=ds, n_shot=1, n_shot_full=100, n_shot_cluster=1, n_neighbors=3, env_array=env,
                device="cuda:0", cluster_backend="device", full_precision=prec, return_mask="mask" in opts,
                search_precision="fp16" if "sp16" in opts else "fp32", knn_per_query="per_query" in opts).eval()
    return net, torch.randn(B, d, generator=g).cuda()


def _weights(N, learnable):
    a = torch.tensor(H.PATTERN)[torch.arange(N) % 7]
    return torch.where(torch.isinf(a), torch.tensor(-2.0), a) if learnable else a


def _call(net, x, entry, arg, opts, N):
    rows = torch.tensor([0, -1, 5], device=x.device)
    if entry == "predict":
        return net.predict(x, arg, leave_out=rows if "leave_out" in opts else None)
    if entry == "predict_loo":
        return net.predict_loo(torch.tensor([7, 0, 21, 3, 12]) if arg == "rows" else None, batch_size=16)
    if entry == "forward_bank":
        out = net.forward_bank(x.requires_grad_(), leave_out=rows if "leave_out" in opts else None)
        if "bwd" in opts:
            g = torch.Generator().manual_seed(B)
            (out[0] if isinstance(out, tuple) else out).backward(torch.randn(B, C, generator=g).to(x.device))
        return out
    if entry == "refresh_bank":
        if arg == "bank_features":
            net.forward_bank(x)
        return net.refresh_bank(rows, x * 0.5 if arg == "feats" else None, 0.5 if arg == "feats" else 0.0)
    if entry == "get_neighbors":
        return net.get_neighbors(x, None if arg == "None" else int(arg))
    if entry == "explain":
        return net.explain(x, torch.arange(B, device=x.device) % C, None if arg == "None" else int(arg))
    if entry == "set_support_weights":
        w = _weights(N, False)
        w = {"short": w[:-1], "nan": w * float("nan"), "inf": -w, "neginf": w, "ok": w}[arg]
        return net.set_support_weights(w, learnable="lw" in opts)
    raise KeyError(entry)


def run_case(nwhead_amd, case_id):
    """-> {"calls", "raises", "out", "state"} of one case.  ``nwhead_amd``: the package under test (or its parent's).  Cached
    workspaces and workspace sizes are dropped before the call, so that what it asks and finds does not depend on earlier
    ones."""
    from nwhead_amd.nwhead.nw import NWNet
    ops = nwhead_amd.ops
    net_name, state, call = case_id.split("/")
    call, *opts = call.split("+")
    entry, _, arg = call.partition("-")
    np.random.seed(0)
    torch.manual_seed(0)
    net, x = _net(NWNet, net_name, opts)
    out, raised, gate = None, None, ops.KNN_FUSED_MIN_SCORE_BYTES
    with torch.no_grad():
        if entry != "precompute":
            if state != "sharded":
                net.precompute()
            if state != "resident":
                net.precompute_sharded()
    if "custom" in opts:                   # (after the banks: a ShardedBank is built for a built-in kernel)
        net.kernel = net.nwhead.kernel = _NegDistance()
    resident = hasattr(net, "full_feat")
    N =net.full_feat.shape[0] if resident else C * NETS[net_name][2] * NETS[net_name][3]
    for kind in ("w", "lw"):
        if kind in opts and entry != "set_support_weights" and resident:
            net.set_support_weights(_weights(N, kind == "lw"), learnable=kind == "lw")
    if "stale" in opts and resident:
        with torch.no_grad():
            net.full_feat.mul_(0.5)
    ops._WS_CACHE.clear()
    ops._WS_BYTES.clear()
    cache = getattr(net, "full_cache", None)
    with _Recorder(ops, q=x, s=getattr(net, "full_feat", None), labels=getattr(net, "full_y", None), bank=cache,
                   entries=ENTRIES) as rec:
        w = net.support_weights if "lw" not in opts else dict(net.named_parameters()).get("support_logw")
        if w is not None:
            rec.roles.setdefault(w.data_ptr(), "row_logw")
        shard = getattr(getattr(net, "sharded_bank", None), "cache", None)
        for role in R.BANK_ROLES if shard is not None else ():
            if getattr(shard, role) is not None:
                rec.roles.setdefault(getattr(shard, role).data_ptr(), "shard." + role)
        try:
            if "open" in opts:
                ops.KNN_FUSED_MIN_SCORE_BYTES = 0
            if entry == "precompute":
                with torch.no_grad():
                    if state != "sharded":
                        net.precompute()
                    if state != "resident":
                        net.precompute_sharded()
            else:
                out = _call(net, x, entry, arg, opts, N)
        except (ValueError, ops.NWHipError, AttributeError) as e:
            raised = f"{type(e).__name__}: {e}"
        finally:
            ops.KNN_FUSED_MIN_SCORE_BYTES = gate
        logw = dict(net.named_parameters()).get("support_logw")
        grads = {"gq": x.grad, "glogw": None if logw is None else logw.grad}
        calls = rec.resolve(grads)
    pair = isinstance(out, tuple) and len(out) == 2 and out[1].dtype == torch.bool
    outs = [t for t in (out if isinstance(out, (tuple, list)) else [out]) if torch.is_tensor(t)]
    if entry in ("precompute", "refresh_bank") and hasattr(net, "full_feat"):     # what the call left in the bank: the labels,
        # the rows a refresh writes and one it does not, and the norms of every row as the prepared bank holds them
        outs += [net.full_y, net.full_feat[[0, 1, 5]]] + [t for t in (net.full_cache.norm2, getattr(net, "full_norm2", None)) if t is not None]
    state = {"rebuilt": getattr(net, "full_cache", None) is not cache, "bank_features": getattr(net, "bank_features", None) is not None,
             "logw_parameter": logw is not None, "weights_set": net.support_weights is not None, "pair": pair}
    return {"calls": calls, "raises": raised, "state": state,
            "out": K.encode([t.detach() for t in outs + [t for t in grads.values() if t is not None]])}
