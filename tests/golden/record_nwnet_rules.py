"""Record what every public entry point of NWNet does in every bank state, for tests/test_nwnet_rules_host.py (no device):

    python tests/golden/record_nwnet_rules.py <root of a checkout of the PARENT of the change under test> tests/golden/nwnet_rules.json

The nets are NWNet(torch.nn.Identity(), C, device="cpu") over a toy dataset; the bank attributes are set by hand for each
state, and the functions of nwhead_amd.ops that nw.py and utils.py reach -- and the sharded bank -- are stubs that note the
call with its distinguishing keywords and return zeros of the right shape, so no kernel runs.  Public methods and attribute
assignment only: the script runs unchanged on the parent.  A cell is <state>/<kernel and weights>/<call>:

  state    r<0 | 1 | s>: no resident bank, one whose full_cache matches, one whose full_cache is stale;
           s<0 | 1>: a sharded bank;  k<0 | 1>: support_eval has what precompute() builds (its knn among it)
  kernel   builtin-none | builtin-constant | builtin-learnable (the support weights) | custom-none (a custom kernel module;
           set_support_weights refuses one, so weights beside it are no state of the net)
  call     CALLS below; EXTRA_IDS: argument errors, on one state

and records the exception ("Type: message") or the stub calls in order, whether full_cache was rebuilt (by identity),
whether bank_features is set, whether support_logw is a parameter and whether the result is an (out, mask) pair.

nwnet_rules.json was recorded from commit 2486763 (before bank_rule: the dozen hand-written bank-state tests).  It must
never be recorded from the tree it is used to test."""
import itertools
import json
import os
import sys
from unittest import mock

import numpy as np
import torch
import torch.nn as nn

B, C, N, D, K = 3, 4, 12, 8, 3
MODES = ("random", "full", "cluster", "ensemble", "knn", "hnsw")
STATES = tuple(f"r{r}s{s}k{k}" for r in "01s" for s in "01" for k in "01")
NETS = ("builtin-none", "builtin-constant", "builtin-learnable", "custom-none")
CALLS = tuple(f"predict-{m}{lo}" for m in MODES for lo in ("", "-leave_out")) \
    + tuple(f"predict-{m}-per_query" for m in ("knn", "hnsw")) \
    + ("predict_loo", "forward_bank", "forward_bank-leave_out", "refresh_bank", "get_neighbors", "get_neighbors-k", "explain",
       "set_support_weights", "set_support_weights-learnable", "set_support_weights-none", "weights_for", "weights_for-graph",
       "predict-full-return_mask", "predict_loo-return_mask", "forward_bank-return_mask")
EXTRA_IDS = tuple("r1s0k1/builtin-none/" + c for c in (
    "set_support_weights-short", "set_support_weights-nan", "set_support_weights-inf", "set_support_weights-learnable-neginf",
    "predict-full-leave_out-short", "predict-full-leave_out-float", "forward_bank-leave_out-short", "refresh_bank-nothing",
    "refresh_bank-bank_features", "get_neighbors-k0", "get_neighbors-kN1"))


def cell_ids():
    return [f"{s}/{n}/{c}" for s, n, c in itertools.product(STATES, NETS, CALLS)] + list(EXTRA_IDS)


def facts(cell_id):
    """The facts of a cell as bank_rule takes them: (entry, its keywords)."""
    state, net, call = cell_id.split("/")
    kernel, weights = net.split("-")
    entry, _, rest = call.partition("-")
    kw = dict(resident=state[1] != "0", sharded=state[3] == "1", searchable=state[5] == "1", builtin_kernel=kernel == "builtin",
              weights=weights)
    if entry == "predict":
        mode, _, opt = rest.partition("-")
        kw.update(mode=mode, leave_out=opt == "leave_out", knn_per_query=opt == "per_query")
    elif entry == "get_neighbors":
        kw.update(k_given=rest == "k")
    return entry, kw


class _Dataset(torch.utils.data.Dataset):
    def __init__(self):
        g = torch.Generator().manual_seed(7)
        self.data, self.targets = torch.randn(N, D, generator=g), [i * C // N for i in range(N)]

    def __len__(self):
        return N

    def __getitem__(self, i):
        return self.data[i], self.targets[i]


class _Dot(nn.Module):
    """A custom kernel module, as the reference accepts."""

    def forward(self, x, y):
        return -torch.cdist(x, y)


class _Stubs:
    """The stubs of one cell and the calls they saw."""

    def __init__(self, net_of):
        self.calls, self.net_of = [], net_of

    def note(self, name, **flags):
        self.calls.append(name + "(" + ",".join(f"{k}={v}" for k, v in flags.items()) + ")")

    def logw(self, w):
        p = dict(self.net_of().named_parameters()).get("support_logw")
        return "none" if w is None else "parameter" if w is p else "detached" if not w.requires_grad else "other"

    def patches(self, ops):
        stubs = self

        class SplitBank:
            def __init__(self, s, labels=None, precision="fp32"):
                stubs.note("SplitBank", labels=labels is not None, precision=precision)
                self.src, self.norm2, self.precision = s, None, precision

            def matches(self, s):
                return s is self.src

            def update_rows(self, support, rows, x, momentum=0.0):
                stubs.note("SplitBank.update_rows", grad=x.requires_grad, momentum=momentum)

        def head(name):
            def fn(q, s, sy, n_classes, *a, **kw):
                cache = a[0] if name == "nw_head_bank" else kw.get("support_cache")
                stubs.note(name, grad=q.requires_grad, support_cache=cache is not None, row_window=kw.get("row_window") is not None,
                           exclude=bool(kw.get("exclude")), row_logw=stubs.logw(kw.get("row_logw")))
                return torch.zeros(len(q), n_classes)
            return fn

        def nw_knn(q, bank, k, *a, rounded=False, support=None, **kw):
            stubs.note("nw_knn", k=k, rounded=rounded, support=support is not None)
            return torch.zeros(len(q), k, dtype=torch.int64)

        def nw_scores(q, s, *a, support_cache=None, **kw):
            stubs.note("nw_scores", support_cache=support_cache is not None)
            return torch.zeros(len(q), s.shape[-2])

        def nw_topk(scores, k, *a, **kw):
            stubs.note("nw_topk", k=k)
            return torch.zeros(len(scores), k, dtype=torch.int64)

        def nw_top_influence(q, s, sy, n_classes, qy, k, *a, support_cache=None, **kw):
            stubs.note("nw_top_influence", k=k, support_cache=support_cache is not None)
            return torch.zeros(len(q), n_classes)

        def knn_route_for(*a, **kw):
            stubs.note("knn_route_for")

        def class_balance_logw(labels, n_classes, *a, **kw):
            stubs.note("class_balance_logw")
            return torch.zeros(len(labels))

        def nw_aggregate(scores, sy, n_classes):
            stubs.note("nw_aggregate")
            return torch.zeros(len(scores), n_classes)

        fns = dict(SplitBank=SplitBank, nw_head=head("nw_head"), nw_head_bank=head("nw_head_bank"), nw_knn=nw_knn,
                   nw_scores=nw_scores, nw_topk=nw_topk, nw_top_influence=nw_top_influence, knn_route_for=knn_route_for,
                   class_balance_logw=class_balance_logw, nw_aggregate=nw_aggregate)
        return [mock.patch.object(ops, k, v) for k, v in fns.items()], SplitBank

    def sharded(self):
        stubs = self

        class Sharded:
            def predict(self, q):
                stubs.note("sharded.predict", grad=q.requires_grad)
                return torch.zeros(len(q), C)

            def predict_knn(self, q, k):
                stubs.note("sharded.predict_knn", k=k)
                return torch.zeros(len(q), C)

            def neighbors(self, q, k):
                stubs.note("sharded.neighbors", k=k)
                return torch.zeros(len(q), k, dtype=torch.int64)

        return Sharded()


def _build(state, kind, stubs, SplitBank):
    """The net of one cell: the bank attributes of ``state`` and the kernel and weights of ``kind``, set by hand."""
    from nwhead_amd.nwhead.nw import NWNet
    from nwhead_amd.nwhead.utils import HNSW, KNN, FeatureDataset, InfiniteUniformClassLoader
    ds = _Dataset()
    net = NWNet(nn.Identity(), C, support_dataset=ds, n_shot=1, n_shot_full=N, n_neighbors=K, device="cpu").eval()
    kernel, weights = kind.split("-")
    if kernel == "custom":
        net.kernel = net.nwhead.kernel = _Dot()
    feat, y = ds.data.clone(), torch.tensor(ds.targets)
    if state[1] != "0":
        net.full_feat, net.full_y = feat, y
        net.full_cache = SplitBank(feat if state[1] == "1" else feat.clone(), labels=y)
    if state[3] == "1":
        net.sharded_bank = stubs.sharded()
    if state[5] == "1":
        se = net.support_eval
        se.full_feat, se.full_y, se.full_meta = feat, y, torch.zeros(N)
        se.full_feat_sep, se.full_y_sep = [feat], [y]
        se.cluster_feat, se.cluster_y = feat[:C].clone(), torch.arange(C)
        se.random_iter = InfiniteUniformClassLoader(FeatureDataset(feat, y, torch.zeros(N)), 1)
        se.knn, se.hnsw = KNN(feat, y, n_neighbors=K), HNSW(feat, y, n_neighbors=K)
        se.knn.bank = se.hnsw.bank = getattr(net, "full_cache", None)
    if weights == "constant":
        net.support_weights = torch.zeros(N)
    if weights == "learnable":
        net.support_logw = nn.Parameter(torch.zeros(N))
    stubs.calls.clear()
    return net


def _call(net, call):
    x, rows = torch.zeros(B, D), torch.tensor([0, -1, 5])
    entry, _, rest = call.partition("-")
    opts = rest.split("-") if rest else []
    if "return_mask" in opts:
        net.return_mask = True
    if entry == "predict":
        if "per_query" in opts:
            net.knn_per_query = True
        lo = None if "leave_out" not in opts else rows[:2] if "short" in opts else rows.float() if "float" in opts else rows
        return net.predict(x, opts[0], leave_out=lo)
    if entry == "predict_loo":
        return net.predict_loo()
    if entry == "forward_bank":
        return net.forward_bank(x, leave_out=None if "leave_out" not in opts else rows[:2] if "short" in opts else rows)
    if entry == "refresh_bank":
        if "bank_features" in opts:
            net.bank_features = x
        return net.refresh_bank(rows, None if opts else x, 0.5)
    if entry == "get_neighbors":
        return net.get_neighbors(x, {"k": K, "k0": 0, "kN1": N + 1}.get(rest))
    if entry == "explain":
        return net.explain(x, torch.zeros(B, dtype=torch.int64))
    if entry == "set_support_weights":
        w = torch.linspace(-1, 1, N)
        w = {"none": None, "short": w[:-1], "nan": w * float("nan"), "inf": w * float("inf")}.get(opts[0] if opts else "", w)
        if "neginf" in opts:
            w[3] = float("-inf")
        return net.set_support_weights(w, learnable="learnable" in opts)
    if entry == "weights_for":
        w = net._weights_for("forward_bank", graph=bool(opts))
        return None if w is None else "parameter" if w is dict(net.named_parameters()).get("support_logw") else "detached"
    raise KeyError(call)


def run_cell(cell_id):
    from nwhead_amd import ops
    state, kind, call = cell_id.split("/")
    holder = {}
    stubs = _Stubs(lambda: holder["net"])
    patches, SplitBank = stubs.patches(ops)
    for p in patches:
        p.start()
    try:
        np.random.seed(0)
        torch.manual_seed(0)
        net = holder["net"] = _build(state, kind, stubs, SplitBank)
        cache, out, raised = getattr(net, "full_cache", None), None, None
        try:
            out = _call(net, call)
        except Exception as e:      # (whatever the call raises is the record: NWHipError, ValueError, AttributeError)
            raised = f"{type(e).__name__}: {e}"
        return {"raises": raised, "calls": list(stubs.calls), "result": out if isinstance(out, str) else None,
                "rebuilt": getattr(net, "full_cache", None) is not cache,
                "bank_features": getattr(net, "bank_features", None) is not None,
                "logw_parameter": "support_logw" in dict(net.named_parameters()),
                "weights_set": net.support_weights is not None,
                "pair": isinstance(out, tuple) and len(out) == 2 and out[1].dtype == torch.bool}
    finally:
        for p in patches:
            p.stop()


def record():
    return {cid: run_cell(cid) for cid in cell_ids()}


def pack(table):
    """The table as the file holds it: every distinct record once, and per cell, in the order of cell_ids(), its index."""
    records = []
    for rec in table.values():
        if rec not in records:
            records.append(rec)
    return {"records": records, "cells": [records.index(table[cid]) for cid in cell_ids()]}


def unpack(packed):
    assert len(packed["cells"]) == len(cell_ids())
    return {cid: packed["records"][i] for cid, i in zip(cell_ids(), packed["cells"])}


if __name__ == "__main__":
    sys.path.insert(0, os.path.abspath(sys.argv[1]))
    table = record()
    from nwhead_amd import ops
    print(f"{len(table)} cells, {sum(r['raises'] is not None for r in table.values())} raise, nwhead_amd from {os.path.dirname(ops.__file__)}")
    with open(sys.argv[2], "w") as fh:
        json.dump(pack(table), fh, indent=None, sort_keys=True, separators=(",", ":"))
        fh.write("\n")
