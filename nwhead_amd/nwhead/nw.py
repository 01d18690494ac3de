"""NWNet / NWHead with the reference's constructor and method surface (nwhead/nw.py:11-289), the
head computed by the HIP kernels in nwhead_amd/csrc/ through ops.nw_head.

Differences that are deliberate (and documented in DESIGN.md):
  * the precomputed bank (full_feat/full_y) stays on the device instead of round-tripping through
    host memory every predict() (reference: nw.py:156,226);
  * 'hnsw' mode is an exact search (hnswlib is not available);
  * there is no CPU execution path: tensors must live on the MI355X.
"""
from typing import NamedTuple

import torch
import torch.nn as nn

from .. import ops
from .kernel import _ScoreModule, get_kernel
from .support import SupportSetEval, SupportSetTrain
from .utils import routed_search


# ---------------------------------------------------------------------- which bank serves a call (DESIGN.md 4.8j has the table)
class Refusal(NamedTuple):
    """bank_rule's "no": the exception to raise, and whether it comes before the entry point does any work (its featurizer
    pass, predict_loo's first batch) or after."""
    kind: type
    text: str
    early: bool = True


# entry point -> how its messages name it
WHAT = {"predict": "predict(x, 'full')", "predict_leave_out": "predict(x, 'full', leave_out=...)", "predict_loo": "predict_loo",
        "forward_bank": "forward_bank", "refresh_bank": "refresh_bank", "get_neighbors": "get_neighbors", "explain": "explain",
        "set_support_weights": "set_support_weights", "weights_for": None, "set_support_values": "set_support_values",
        "predict_values": "predict_values", "predict_loo_values": "predict_loo_values", "forward_values": "forward_values"}
# entry point -> why it needs ONE resident bank: the head over a row window, the top-influence windows, one weight per row
_ROWS_OF = {"explain": "the row windows of ops.nw_top_influence are rows", "set_support_weights": "the weights are rows",
            "set_support_values": "the values are rows"}


def bank_rule(entry, what=None, *, resident, sharded, searchable=False, builtin_kernel=True, weights="none", mode="full",
              knn_per_query=False, leave_out=False, k_given=True):
    """Which bank serves a call of NWNet: "resident" (precompute()'s full_feat / full_y / full_cache), "sharded"
    (precompute_sharded()'s ShardedBank), "supports" (what support_eval builds per call), "missing" (no bank: the read of
    the attribute fails with AttributeError) -- or the Refusal to raise.  Over plain facts: ``resident`` (full_feat is
    there), ``sharded`` (sharded_bank is set), ``searchable`` (support_eval has its knn: precompute() has run),
    ``builtin_kernel`` (a get_kernel score module), ``weights`` ("none" | "constant" | "learnable"), and of the call
    ``mode``, ``knn_per_query``, ``leave_out`` (given or not) and ``k_given`` (get_neighbors).  ``entry``: a key of WHAT;
    ``what`` names the caller in a message where the entry has no name of its own ("weights_for")."""
    what = what or WHAT[entry]
    if entry == "predict" and leave_out:
        if mode != 'full':
            return Refusal(ops.NWHipError, f"predict(x, '{mode}', leave_out=...): only mode='full' over precompute()'s bank "
                                           "leaves rows out (the other modes build their support per call)")
        entry, what = "predict_leave_out", WHAT["predict_leave_out"]
    if entry == "predict":
        if mode == 'full' and sharded:
            return bank_rule("weights_for", what, resident=resident, sharded=sharded, weights=weights)._replace(early=False) \
                if weights != "none" else "sharded"
        if mode in ('knn', 'hnsw') and sharded and not searchable:
            # a sharded bank and no precompute(): every query over its own neighbours of the whole bank
            return "sharded" if knn_per_query else Refusal(
                ops.NWHipError, f"predict(x, '{mode}') over a sharded bank needs NWNet(knn_per_query=True): the shared-support "
                "form, which pools every query's neighbours, would have to gather their feature rows across the ranks", False)
        # (the rows come from support_eval, which has them once precompute() has run: 'full' hands on ITS full_feat)
        return "missing" if not searchable else "resident" if mode == 'full' else "supports"
    if entry == "get_neighbors":
        if sharded and not resident:
            return "sharded" if k_given else Refusal(
                ops.NWHipError, "get_neighbors over a sharded bank needs k (1 <= k <= 32): the full ordering of a sharded bank "
                "is not available", False)
        return "resident" if resident else "missing"
    if entry == "weights_for":
        if weights != "none" and sharded:
            return Refusal(ops.NWHipError, f"{what}: support weights are set and the bank is sharded; a sharded bank has no "
                                           "weights (set_support_weights(None), or precompute())")
        return "resident"
    # the entry points over ONE resident bank.  explain and set_support_weights look past a sharded bank when there is a
    # resident one as well, and so does set_support_values; the head over a row window (predict_loo, leave_out, forward_bank,
    # refresh_bank) and the value head (predict_values, predict_loo_values, forward_values) do not
    if sharded and not (resident and entry in _ROWS_OF):
        return Refusal(ops.NWHipError, f"{what}: a sharded bank is not served ({_ROWS_OF.get(entry, 'a row window is rows')} of "
                                       "one resident bank); call precompute()")
    if not resident:
        return Refusal(ops.NWHipError, f"{what} needs the bank of precompute()")
    if not builtin_kernel:
        # (late: the bank getter says it, after the featurizer pass of forward_bank and leave_out, with predict_loo's first
        # batch -- none for no rows; explain and set_support_weights ask once, before anything else)
        return Refusal(ops.NWHipError, f"{what} needs one of the built-in score kernels", False)
    return "resident"


class _ChannelsLast(nn.Module):
    """An inference copy of a backbone kept in channels_last layout; 4-D inputs are converted on the way in."""

    def __init__(self, inner):
        super().__init__()
        self.inner = inner.to(memory_format=torch.channels_last)

    def forward(self, x):
        return self.inner(x.contiguous(memory_format=torch.channels_last) if x.dim() == 4 else x)


class NWHead(nn.Module):
    """forward(x:(B,d), sx:(N,d)|(B,N,d), sy:(N,)|(B,N)) -> (B, n_classes) log-probabilities."""

    def __init__(self, kernel, n_classes, validate_labels=False):
        super().__init__()
        self.kernel = kernel
        self.n_classes = n_classes
        # not in the reference: its F.one_hot (nw.py:276) refuses support labels >= n_classes; here that check costs a device
        # round trip per call, so it is an option (on under NWNet(debug_mode=True)); without it such supports are skipped
        self.validate_labels = bool(validate_labels)

    def forward(self, x, sx, sy, return_weights=False, support_norm2=None, support_cache=None):
        if not isinstance(self.kernel, _ScoreModule):
            # any other callable kernel module, as the reference accepts (nw.py:256-264, :277-283): its scores (torch
            # ops on the device, with their autograd history), then the softmax / aggregation / log tail in HIP
            if return_weights:
                raise NotImplementedError("return_weights needs one of the built-in score functions (get_kernel)")
            b = len(x)
            sxe = sx[None].expand(b, *sx.shape) if sx.dim() == x.dim() else sx       # nw.py:277-279
            scores = self.kernel(x.unsqueeze(1), sxe).squeeze(1)                      # nw.py:281-283
            return ops.nw_aggregate(scores, sy, self.n_classes)
        return ops.nw_head(x, sx, sy, self.n_classes, self.kernel.kind, self.kernel._logit_scale(),
                           return_weights=return_weights, support_norm2=support_norm2,
                           support_cache=support_cache, validate_labels=self.validate_labels)


class NWNet(nn.Module):
    def __init__(self, featurizer, n_classes, support_dataset=None, feat_dim=None, proj_dim=0,
                 kernel_type='euclidean', train_type='random', n_way=None, n_shot=1,
                 n_shot_random=1, n_shot_full=100, n_shot_cluster=1, n_neighbors=10,
                 env_array=None, debug_mode=False, device='cuda:0', return_mask=False, cluster_backend='auto',
                 loader_workers=0, pin_memory=False, knn_per_query=False, full_precision="fp32",
                 search_precision="fp32", balance_full="truncate"):
        super().__init__()
        # not in the reference: how the 'full' bank gets its flat class prior.  "truncate" (the reference): every class is cut
        # to the rarest class's row count.  "weights": every class keeps its first min(n_shot_full, n_c) rows and precompute()
        # sets support weights -log n_c (ops.class_balance_logw), which predict('full'), predict_loo and forward_bank honour
        if balance_full not in ("truncate", "weights"):
            raise ValueError(f"balance_full must be 'truncate' or 'weights', got {balance_full!r}")
        self.balance_full = balance_full
        self.support_weights = None
        self.support_values = None     # ops.BankValues over the rows of precompute()'s bank (set_support_values), or None
        # not in the reference: "fp16" serves predict(x, 'full') from a half-precision bank (ops.SplitBank(precision="fp16"):
        # bank and query features rounded to fp16, half the bytes, a third of the matrix-core work); "fp32" is the parity path
        if full_precision not in ("fp32", "fp16"):
            raise ValueError(f"full_precision must be 'fp32' or 'fp16', got {full_precision!r}")
        self.full_precision = full_precision
        # not in the reference: "fp16" (needs full_precision="fp16") makes get_neighbors(x, k <= 32) and the neighbour selection
        # of predict(x, 'knn' | 'hnsw') the exact search over the fp16-rounded features (ops.nw_knn(rounded=True)) whenever
        # the bank can serve it; "fp32" is the fp32-grade search
        if search_precision not in ("fp32", "fp16"):
            raise ValueError(f"search_precision must be 'fp32' or 'fp16', got {search_precision!r}")
        if search_precision == "fp16" and full_precision != "fp16":
            raise ValueError("search_precision='fp16' searches the half-precision bank: it needs full_precision='fp16'")
        self.search_precision = search_precision
        self.knn_per_query = bool(knn_per_query)  # not in the reference: 'knn' / 'hnsw' modes give every query ITS OWN neighbours
        self.cluster_backend = cluster_backend   # not in the reference: where 'cluster' mode's k-means runs (utils.compute_clusters)
        # not in the reference either (its bank loaders are single-process, support.py:164-165): DataLoader workers and
        # pinned staging for the loaders precompute() featurises the bank from; same row order whatever they are
        self.loader_workers, self.pin_memory = int(loader_workers), bool(pin_memory)
        if support_dataset is not None:
            assert hasattr(support_dataset, 'targets'), 'Support set must have .targets attribute'
        if proj_dim > 0:
            assert feat_dim is not None, 'Feature dimension must be specified'
            featurizer = nn.Sequential(featurizer, nn.Linear(feat_dim, proj_dim))
        self.featurizer = featurizer
        self.n_classes, self.train_type, self.n_way = n_classes, train_type, n_way
        self.n_shot, self.n_shot_random, self.n_shot_full = n_shot, n_shot_random, n_shot_full
        self.n_shot_cluster, self.n_neighbors = n_shot_cluster, n_neighbors
        self.env_array, self.debug_mode = env_array, debug_mode
        self.device, self.return_mask = device, return_mask
        # registered twice on purpose: reference state_dicts carry both kernel.* and nwhead.kernel.*
        self.kernel = get_kernel(kernel_type)
        self.nwhead = NWHead(self.kernel, n_classes, validate_labels=bool(debug_mode))
        if support_dataset is not None:
            self.support_train = SupportSetTrain(support_dataset, n_classes, train_type, n_shot,
                                                 n_way=n_way, env_array=env_array)
            self.process_support_eval(support_dataset)

    # ------------------------------------------------------------------ eval-mode BatchNorm folding
    def enable_bn_folding(self, on=True, channels_last=True):
        """Inference (precompute / predict / get_neighbors, featurizer in eval mode) then runs a copy of the
        featurizer whose conv -> BatchNorm pairs are single convolutions (model.fold_batchnorm, SURVEY 8f
        N1), kept in channels_last layout (MIOpen's faster fp32 path: ResNet-18 over 64 images @224
        3.81 -> 3.55 ms folded -> 3.22 ms folded + channels_last, features equal to 3e-7 relative).  The copy
        is rebuilt by precompute() and dropped by train(); it is not part of state_dict()."""
        object.__setattr__(self, '_fold_bn', bool(on))
        object.__setattr__(self, '_fold_cl', bool(channels_last))
        object.__setattr__(self, '_folded', None)

    def _weights_signature(self):
        """Changes whenever a parameter or buffer of the featurizer is written in place (optimizer step,
        load_state_dict, BatchNorm statistics) or replaced: the folded inference copy is rebuilt then.  (torch's fused
        optimizers do not advance version counters; train(), which every training loop passes through, drops the copy.)"""
        from ..model.backbones import tensor_signature
        return tensor_signature(self.featurizer)

    def _eval_featurizer(self, rebuild=False):
        if not getattr(self, '_fold_bn', False) or self.featurizer.training:
            return self.featurizer
        sig = self._weights_signature()
        if rebuild or getattr(self, '_folded', None) is None or getattr(self, '_folded_sig', None) != sig:
            object.__setattr__(self, '_folded_sig', sig)
            from ..model.backbones import fold_batchnorm, folded_stays_nchw
            folded = fold_batchnorm(self.featurizer)
            if getattr(self, '_fold_cl', False) and not folded_stays_nchw(folded):
                folded = _ChannelsLast(folded)
            object.__setattr__(self, '_folded', folded)
        return self._folded

    def train(self, mode=True):
        if mode:                                         # the weights are about to change
            object.__setattr__(self, '_folded', None)
            self.sharded_bank = None                     # a shard featurised with the old weights must not serve 'full'
        return super().train(mode)

    def load_state_dict(self, *args, **kwargs):
        object.__setattr__(self, '_folded', None)
        self.sharded_bank = None
        return super().load_state_dict(*args, **kwargs)

    # ------------------------------------------------------------------ evaluation bank
    def process_support_eval(self, support_dataset):
        self.support_eval = SupportSetEval(support_dataset, self.n_classes, self.n_shot_random,
                                           self.n_shot_full, n_shot_cluster=self.n_shot_cluster,
                                           n_neighbors=self.n_neighbors, env_array=self.env_array,
                                           knn_per_query=self.knn_per_query, search_precision=self.search_precision,
                                           cluster_backend=self.cluster_backend, loader_workers=self.loader_workers,
                                           pin_memory=self.pin_memory, balance_full=self.balance_full)

    @torch.no_grad()
    def _compute_all_support_feats(self):
        """Featurise every environment's balanced bank in loader order; rows stay on self.device."""
        per_env = []
        featurizer = self._eval_featurizer(rebuild=True)
        for loader in self.support_eval.support_loaders:
            f, y, m = [], [], []
            for img, label, meta in loader:
                f.append(featurizer(img.to(self.device, non_blocking=self.pin_memory)).detach())
                y.append(label.to(self.device))
                m.append(meta.to(self.device))
            per_env.append((torch.cat(f), torch.cat(y), torch.cat(m)))
        feats, labels, meta = (torch.cat([e[k] for e in per_env]) for k in range(3))
        return (feats, labels, meta, [e[0] for e in per_env], [e[1] for e in per_env],
                [e[2] for e in per_env])

    def precompute(self):
        assert not self.featurizer.training
        info = self._compute_all_support_feats()
        self.sharded_bank = None                     # predict('full') serves the bank built here
        self.full_feat, self.full_y = info[0], info[1]
        # norms + split-fp16 (or fp16) rows for predict('full')
        self.full_cache = ops.SplitBank(self.full_feat, labels=self.full_y, precision=self.full_precision)
        self.full_norm2 = self.full_cache.norm2
        self.support_eval.build_infer_iters(*info)
        self.support_eval.knn.bank = self.support_eval.hnsw.bank = self.full_cache   # neighbour search over the same bank
        self.support_weights = None                  # weights are per row of the bank they were set for
        self.support_values = None                   # ... and so are values
        self._parameters.pop('support_targets', None)   # ... learnable ones with their parameter
        self._parameters.pop('support_bank', None)      # ... and learnable rows belong to the bank they were registered for
        if self.balance_full == "weights":
            self.set_support_weights(ops.class_balance_logw(self.full_y, self.n_classes))

    @property
    def support_weights(self):
        """The (N,) fp32 log-weights in force, or None -- as a constant: of a learnable set (set_support_weights(...,
        learnable=True)) the current values of the parameter ``support_logw``, detached."""
        p = self._parameters.get('support_logw')
        return p.detach() if p is not None else self.__dict__.get('_support_weights')

    @support_weights.setter
    def support_weights(self, w):
        self._parameters.pop('support_logw', None)       # a learnable set ends with the weights it was registered for
        self.__dict__['_support_weights'] = w

    def set_support_weights(self, log_w=None, learnable=False):
        """Not in the reference: a prior weight per row of precompute()'s bank.  ``log_w``: (N,) float tensor over the rows of
        ``full_feat``, the natural logs a_j = log w_j; ``None`` clears them.  The 'full' head becomes the head of
        score + a (ops.nw_head_window has the formula): -inf switches a row off (soft deletion, label-noise screening after
        predict_loo, "what if these supports were gone", a subgroup or environment of the bank -- any subset, no rebuild),
        ops.class_balance_logw(full_y, n_classes) gives an unbalanced bank a flat class prior, finite values are
        importance / confidence / recency weights.  Checked once, here (one device synchronisation): NaN or +inf raise
        ValueError.  The weights are a constant: no gradient flows to them.

        ``learnable=True`` makes them LEARNED instead (importance / confidence weights against label noise, data valuation,
        a recency decay): they are registered as the nn.Parameter ``support_logw`` -- in parameters() and state_dict() from
        this call on, not before -- forward_bank passes the parameter with its graph, so a loss on its output puts a
        gradient on ``support_logw`` (ops.nw_head_bank: no (B, N) matrix; only the weights learning skips the second pass
        over the bank), while predict('full'), predict_loo and leave_out read the current values detached;
        ``support_weights`` is that detached view.  The values must be finite: an optimizer's weight decay turns -inf
        into NaN -- to switch rows off, keep a constant -inf mask OUTSIDE the parameter (ops.nw_head_bank(...,
        row_logw=net.support_logw + mask)).  precompute() clears learnable weights like any others, parameter included:
        set them again afterwards and rebuild the optimizer's parameter group.  A full_precision="fp16" bank has no route
        for this gradient: forward_bank raises NWHipError.  ``learnable=False`` is the behaviour described above, unchanged.

        Honoured by predict(x, 'full') with and without leave_out, by predict_loo, by forward_bank and by the value head
        (predict_values, predict_loo_values).  Kept by
        refresh_bank (rows keep their identity); cleared by precompute().  NOT seen by get_neighbors, explain and the
        other inference modes ('random', 'cluster', 'ensemble', 'knn', 'hnsw'), which read the bank's features as they are.
        A sharded bank is refused (NWHipError), as is a custom kernel module."""
        if log_w is None:
            self.support_weights = None
            return
        self._served("set_support_weights")
        # (a copy of its own: later writes to the caller's tensor do not get past the check below)
        w = torch.as_tensor(log_w).detach().to(device=self.full_feat.device, dtype=torch.float32, copy=True).contiguous()
        if w.shape != (self.full_feat.shape[0],):
            raise ValueError(f"set_support_weights: log_w must be ({self.full_feat.shape[0]},), one value per bank row; got "
                             f"{tuple(w.shape)}")
        if bool((torch.isnan(w) | (w == float("inf"))).any()):
            raise ValueError("set_support_weights: log_w holds NaN or +inf (finite values and -inf only)")
        if learnable and not bool(torch.isfinite(w).all()):
            raise ValueError("set_support_weights(learnable=True): log_w must be finite -- an optimizer's weight decay turns "
                             "-inf into NaN; switch rows off by adding a constant -inf mask outside the parameter")
        self.support_weights = None if learnable else w   # (drops a parameter of an earlier call)
        if learnable:
            self.support_logw = nn.Parameter(w)           # the values live in the parameter alone

    def set_bank_learnable(self, on=True):
        """Not in the reference: make the ROWS of precompute()'s bank LEARNED (prototypes, a condensed support set, a memory
        bank trained end to end rather than by momentum refresh).  After precompute(): registers the nn.Parameter
        ``support_bank``, which shares ``full_feat``'s storage -- in parameters() and state_dict() from this call on, not
        before; rebuild the optimizer's parameter group.  forward_bank then passes the parameter with its graph
        (ops.nw_head_bank(support_grad=True): no (B, N) matrix), so a loss on its output puts a gradient on
        ``support_bank``, with ``leave_out`` too.  forward_values does the same for the value head
        (ops.nw_head_values_bank(support_grad=True)): the rows are then the learnable KEYS of a key-value
        memory, beside learnable values (``support_targets``) and weights or on their own.  After the optimizer wrote the
        rows, every entry point that reads the bank re-prepares it in place first (ops.SplitBank.refresh: no rebuild, no allocation); predict('full'), predict_loo,
        get_neighbors and explain read the rows detached, and refresh_bank keeps working (it writes in place).  Cleared by
        precompute() and by ``set_bank_learnable(False)``, like ``support_logw``.  A sharded bank, a missing bank and a custom
        kernel module are refused (NWHipError) as for forward_bank; a full_precision="fp16" bank or one whose labels are not
        class-sorted takes ops.nw_head's matrix route without ``leave_out`` or weights and is refused with them."""
        self._parameters.pop('support_bank', None)
        if not on:
            return
        self._served("forward_bank")
        self.support_bank = nn.Parameter(self.full_feat)     # (the same storage and the same in-place version counter)

    def _weights_for(self, what, graph=False):
        """The support weights for a call over precompute()'s resident bank, or None; a sharded bank in front of it refuses.
        ``graph``: learnable weights as the parameter itself, for a call that differentiates (forward_bank)."""
        self._served("weights_for", what)
        return self._weights(graph)

    def _weights(self, graph=False):
        """_weights_for without the question: for the entry points, which have asked bank_rule for their bank already."""
        w = self._parameters.get('support_logw') if graph else None
        return self.support_weights if w is None else w

    def _served(self, entry, what=None, early_only=False, **call):
        """bank_rule's answer for this net and this call (``call``: the call's own facts -- mode, leave_out, k_given); the
        net's facts are gathered here and nowhere else.  A Refusal is raised (``early_only``: one that comes before the
        featurizer pass; any other is left to the same question after it)."""
        weights = "learnable" if self._parameters.get('support_logw') is not None else \
            "none" if self.__dict__.get('_support_weights') is None else "constant"
        served = bank_rule(entry, what, resident=hasattr(self, 'full_feat'), sharded=getattr(self, 'sharded_bank', None) is not None,
                           searchable=hasattr(getattr(self, 'support_eval', None), 'knn'),
                           builtin_kernel=isinstance(self._modules['kernel'], _ScoreModule),    # (self.kernel, without __getattr__)
                           weights=weights, knn_per_query=self.knn_per_query, **call)
        if isinstance(served, Refusal) and (served.early or not early_only):
            raise served.kind(served.text)
        return served

    def _result(self, out):
        """``out`` as the entry points return it: with return_mask, beside the mask of queries that were served (all)."""
        return (out, torch.full((len(out),), True)) if self.return_mask else out

    @torch.no_grad()
    def precompute_sharded(self, group=None, partial_fn=None, merge_fn=None, search_fn=None, knn_merge_fn=None):
        """'full' inference over a bank sharded across the ranks of `group`: this
        rank featurises ONLY rows [lo, hi) of the balanced, class-sorted bank -- the row order of
        precompute() (environments in order, support.py loader order inside) -- and keeps them resident
        as a ShardedBank; the bank is never gathered.  predict(x, 'full') then exchanges one packed
        partial per query batch.
        The neighbour search works over the shards as well: get_neighbors(x, k) returns global rows in precompute()'s row
        order, and predict(x, 'knn' | 'hnsw') with knn_per_query=True evaluates every query over its own n_neighbors
        nearest supports of the whole bank (ShardedBank.neighbors / predict_knn, k <= 32).  The reference's form of
        those two modes pools the neighbours of ALL queries of a batch into one shared support; over a sharded bank that
        would need the neighbours' feature rows gathered across the ranks, which is not done: with knn_per_query=False they
        raise.  The remaining inference modes still need precompute().
        partial_fn / merge_fn / search_fn / knn_merge_fn: compute hooks for the CPU tests (see sharded.ShardedBank)."""
        import torch.distributed as dist
        from torch.utils.data import DataLoader, Subset
        from ..sharded import ShardedBank, shard_bounds
        assert not self.featurizer.training
        world = dist.get_world_size(group) if dist.is_initialized() else 1
        rank = dist.get_rank(group) if dist.is_initialized() else 0
        datasets = self.support_eval.full_datasets
        lo, hi = shard_bounds(sum(len(ds) for ds in datasets), world, rank)
        featurizer = self._eval_featurizer(rebuild=True)
        feats, labels, start = [], [], 0
        for ds in datasets:                                   # this rank's rows of every environment
            a, b = max(lo, start) - start, min(hi, start + len(ds)) - start
            start += len(ds)
            if a >= b:
                continue
            for img, label, _meta in DataLoader(Subset(ds, range(a, b)), batch_size=128, shuffle=False,
                                                num_workers=self.loader_workers, pin_memory=self.pin_memory):
                feats.append(featurizer(img.to(self.device, non_blocking=self.pin_memory)).detach())
                labels.append(label.to(self.device))
        d = feats[0].shape[1] if feats else featurizer(ds[0][0][None].to(self.device)).shape[1]
        feat = torch.cat(feats) if feats else torch.empty(0, d, device=self.device)
        y = torch.cat(labels) if labels else torch.empty(0, dtype=torch.int64, device=self.device)
        self.sharded_bank = ShardedBank(feat, y, self.n_classes, self.kernel.kind, self.kernel._logit_scale(),
                                        group=group, partial_fn=partial_fn, merge_fn=merge_fn,
                                        precision=self.full_precision, row_lo=lo, search_fn=search_fn,
                                        knn_merge_fn=knn_merge_fn, search_precision=self.search_precision)
        return self.sharded_bank

    def _resident_bank(self, entry=None, device=None, rebuild=True, rows=None):
        """precompute()'s bank -- (full_feat, full_y, SplitBank), on ``device`` when one is given -- for an entry point
        bank_rule serves from it; ``entry``: the rule is asked here (NWHipError with the reason: a sharded bank, no bank, a
        custom kernel module), None: the caller has asked.  ``rows``: the (features, labels) predict('full') got from
        support_eval.  The one reader of ``full_cache``: a SplitBank that is not of these rows as they stand (full_feat
        was replaced or updated since precompute()) is rebuilt -- or, with ``rebuild=False`` (get_neighbors, explain, which
        have a route without a bank), left alone and None comes back in its place."""
        if entry is not None:
            self._served(entry)
        sfeat, sy = (self.full_feat, self.full_y) if rows is None else rows
        if device is not None:
            sfeat, sy = sfeat.to(device), sy.to(device)
        cache = getattr(self, 'full_cache', None)
        if cache is not None and not cache.matches(sfeat):
            # learnable rows the optimizer wrote (the same tensor, a later version): every prepared form again, in place
            if (self._parameters.get('support_bank') is not None and cache.sorted_rows is None
                    and cache._src[:2] == (sfeat.data_ptr(), tuple(sfeat.shape))):
                cache.refresh(sfeat)
            else:
                cache = None
        if cache is None and rebuild:
            cache = self.full_cache = ops.SplitBank(sfeat, labels=sy, precision=self.full_precision)
        return sfeat, sy, cache

    @staticmethod
    def _leave_out_window(rows, qfeat, what):
        """``leave_out`` (bank row per query, -1: none) as ops.nw_head's excluded row window [row, row + 1); -1 is the empty
        excluded window [0, 0)."""
        rows = torch.as_tensor(rows, device=qfeat.device)
        if rows.shape != (qfeat.shape[0],) or rows.is_floating_point() or rows.dtype == torch.bool:
            raise ValueError(f"{what}: leave_out is a ({qfeat.shape[0]},) integer tensor: the bank row of each query, or -1")
        lo = rows.clamp(min=0)
        return lo, torch.where(rows < 0, lo, lo + 1)

    def _predict_leave_out(self, qfeat, rows, entry):
        """The 'full' head of the featurised queries ``qfeat`` over precompute()'s bank, query b without bank row rows[b]
        (-1: with every row): ops.nw_head's row window [row, row + 1), excluded."""
        what = WHAT[entry]
        sfeat, sy, cache = self._resident_bank(entry, qfeat.device)
        window = self._leave_out_window(rows, qfeat, what)
        with torch.no_grad():
            return ops.nw_head(qfeat.detach(), sfeat, sy, self.n_classes, self.kernel.kind, self.kernel._logit_scale(),
                               support_cache=cache, row_window=window, exclude=True, row_logw=self._weights())

    def forward_bank(self, x, leave_out=None):
        """Not in the reference: the 'full' head at TRAINING time -- log-probabilities of ``self.featurizer(x)`` over
        precompute()'s bank, differentiable in the featurizer, the projection and a clip scale (ops.nw_head_bank: the query
        gradient is computed without a (B, N) matrix and without a support gradient).  The featurizer is taken as it is,
        not the folded eval copy.  ``leave_out``: (B,) int64, the bank row of each query or -1 for none -- query b is
        predicted without that row (a leave-one-out training loss over the bank's own samples).  Honours return_mask.

        The bank is a CONSTANT here: it holds the features of the weights precompute() saw and goes stale as the weights
        move; the caller decides when to call precompute() again, or writes each batch's features back with
        refresh_bank(rows) -- they are kept, detached, in ``bank_features`` (a view, not a copy).  Support weights
        (set_support_weights) are honoured: as a constant, or, set with learnable=True, as the parameter ``support_logw``
        with its graph (a gradient lands on it).  After set_bank_learnable() the rows themselves are the parameter
        ``support_bank`` and get a gradient as well.  A sharded bank, a missing bank and a custom kernel
        module are refused (NWHipError), like predict_loo.  A full_precision="fp16" bank or a bank whose labels are not
        class-sorted takes ops.nw_head's route through the score matrix without ``leave_out`` and is refused with it."""
        what = WHAT["forward_bank"]
        self._served("forward_bank", early_only=True)      # (a sharded or missing bank: no featurizer pass)
        qfeat = self.featurizer(x)
        self.bank_features = qfeat.detach()
        sfeat, sy, cache = self._resident_bank("forward_bank", qfeat.device)
        window = None if leave_out is None else self._leave_out_window(leave_out, qfeat, what)
        rows = self._parameters.get('support_bank')     # learnable rows: the parameter with its graph
        learn = {} if rows is None else {"support_grad": True}
        out = ops.nw_head_bank(qfeat, sfeat if rows is None else rows, sy, self.n_classes, cache, self.kernel.kind,
                               self.kernel._logit_scale(), row_window=window, exclude=window is not None,
                               row_logw=self._weights(graph=True), **learn)
        return self._result(out)

    def refresh_bank(self, rows, feats=None, momentum=0.0):
        """Not in the reference: write fresh features into rows of precompute()'s bank IN PLACE (ops.SplitBank.update_rows:
        one launch, R rows read and written, no backbone pass, no rebuild of the bank, no host synchronisation) -- the step
        of memory-bank training after forward_bank(x, leave_out=rows), backward and the optimizer step.  ``rows``: (R,)
        integer tensor, the bank row of each feature row (-1 or a row past the bank: skipped; of repeated rows the last
        wins); ``feats``: (R, feat_dim), default the features of the last forward_bank, ``bank_features``, which is then
        cleared; ``momentum`` in [0, 1): the row becomes momentum * old + (1 - momentum) * new, 0 replaces it.  The labels
        of the rows do not change.  A sharded bank, a missing bank and a custom kernel module raise as for forward_bank; a
        bank with several environments' unsorted labels or too few rows for prepared forms is refused (NWHipError).

        What follows the refresh: predict('full') (with leave_out too), forward_bank and predict_loo; get_neighbors and
        explain over the bank; the 'knn' / 'hnsw' / 'random' modes, which read the same tensor.  What does not: the cluster
        centroids and the per-environment copies of 'ensemble' keep precompute()'s features until it runs again."""
        if feats is None:
            feats, self.bank_features = getattr(self, 'bank_features', None), None
            if feats is None:
                raise ops.NWHipError(f"{WHAT['refresh_bank']}: no features to write: call forward_bank first, or pass feats")
        sfeat, _sy, cache = self._resident_bank("refresh_bank", feats.device)
        cache.update_rows(sfeat, torch.as_tensor(rows, device=sfeat.device), feats.detach(), momentum)

    def predict_loo(self, rows=None, batch_size=256):
        """Not in the reference: leave-one-out log-probabilities of the bank's own rows, (len(rows), n_classes) -- row i of
        precompute()'s bank predicted from every row but itself (train-set accuracy without the self-match, label-noise
        screening, model selection by LOO likelihood).  ``rows``: (R,) int64 bank rows, default all of them.  The queries
        are full_feat[rows]: no featurizer pass; batches of ``batch_size``.  The exclusion happens inside the tile kernel
        (ops.nw_head_window), before the softmax -- subtracting the self term afterwards cancels to nothing once the
        nearest other row is far.  A full_precision="fp16" bank, and a bank whose labels are not class-sorted (several
        environments), take ops.nw_head_window's score-matrix route: same result, a (batch, N) matrix per batch.
        Honours return_mask like predict.  A sharded bank is not served: NWHipError."""
        self._served("predict_loo", early_only=True)     # (a custom kernel module is refused by the first batch, if any)
        N = self.full_feat.shape[0]
        rows = torch.arange(N, device=self.full_feat.device) if rows is None else torch.as_tensor(rows, device=self.full_feat.device)
        outs = [self._predict_leave_out(self.full_feat[r], r, 'predict_loo') for r in rows.split(max(int(batch_size), 1))]
        out = torch.cat(outs) if outs else torch.empty(0, self.n_classes, device=self.full_feat.device)
        return self._result(out)

    def set_support_values(self, values=None, learnable=False):
        """Not in the reference: a real-valued TARGET ROW per row of precompute()'s bank, for predict_values /
        predict_loo_values -- Nadaraya-Watson regression over the resident bank (an age, a pose, a box, an embedding to
        retrieve), soft / smoothed / mixup / distilled or multi-hot labels, or any per-row attribute carried through the
        softmax (expected metadata or loss of the neighbours).  ``values``: (N, T) float tensor over the rows of
        ``full_feat``, every entry finite; ``None`` clears them.  Prepared once, here, as an ops.BankValues (``support_values``:
        an fp32 copy and its split-fp16 form) from a copy of the caller's tensor: later writes to that tensor are not seen;
        to change value rows, call this again.  Kept by refresh_bank (rows keep their identity); cleared by precompute().
        A sharded bank, a missing bank and a custom kernel module are refused (NWHipError), like set_support_weights.

        ``learnable=True`` makes the values LEARNED (soft labels corrected against label noise, target prototypes, distilled
        targets): they are registered as the nn.Parameter ``support_targets``, (N, T) fp32 -- in parameters() and
        state_dict() from this call on, not before, like ``support_logw`` -- forward_values passes them with their graph
        (ops.nw_head_values_bank(support_grad=True): no (B, N) matrix), and every value entry point re-prepares the
        BankValues in place (BankValues.refresh) when the parameter was written since -- an optimizer step, a
        load_state_dict.  predict_values / predict_loo_values read the current values detached.  precompute() and
        set_support_values(None) drop the parameter: set the values again and rebuild the optimizer's parameter group."""
        if values is None:
            self._parameters.pop('support_targets', None)
            self.support_values = None
            return
        self._served("set_support_values")
        self._parameters.pop('support_targets', None)    # a learnable set ends with the values it was registered for
        sfeat, _sy, cache = self._resident_bank()
        v = torch.as_tensor(values)
        if v.dim() != 2 or v.shape[0] != sfeat.shape[0] or v.shape[1] < 1 or not v.is_floating_point():
            raise ValueError(f"set_support_values: values must be ({sfeat.shape[0]}, T) floats, T >= 1: one row per bank row; got "
                             f"{tuple(v.shape)} {v.dtype}")
        if learnable:
            self.support_targets = nn.Parameter(v.detach().to(device=sfeat.device, dtype=torch.float32, copy=True).contiguous())
            self.support_values = ops.BankValues(self.support_targets, cache)
        else:
            self.support_values = ops.BankValues(v.detach().to(device=sfeat.device, copy=True), cache)

    def _values(self):
        """``support_values`` for a call, or None: learnable values written since they were prepared (an optimizer step) are
        re-prepared in place first."""
        vals = getattr(self, 'support_values', None)
        if vals is not None and self._parameters.get('support_targets') is not None and vals.stale():
            vals.refresh()
        return vals

    def _values_head(self, qfeat, rows, log, entry):
        """ops.nw_head_values of the featurised queries ``qfeat`` over precompute()'s bank and the values set for it, query b
        without bank row rows[b] (None: no window); constant support weights are honoured, learnable ones read detached."""
        what = WHAT[entry]
        sfeat, _sy, cache = self._resident_bank(entry, qfeat.device)
        vals = self._values()
        if vals is None:
            raise ops.NWHipError(f"{what}: no values are set for the bank: call set_support_values (precompute() clears them)")
        window = None if rows is None else self._leave_out_window(rows, qfeat, what)
        with torch.no_grad():
            return ops.nw_head_values(qfeat.detach(), sfeat, cache, vals, self.kernel.kind, self.kernel._logit_scale(),
                                      row_window=window, exclude=window is not None, row_logw=self._weights(), log=log)

    def predict_values(self, x, leave_out=None, log=False):
        """Not in the reference: the VALUE head over precompute()'s bank -- (B, T) fp32, the softmax-weighted mean of the
        value rows of set_support_values under the configured kernel (ops.nw_head_values: no (B, N) matrix on the fused
        route; a full_precision="fp16" bank or one whose labels are not class-sorted goes through the score matrix).  The
        eval featurizer runs on ``x``.  ``leave_out``: (B,) int64, the bank row of each query or -1 for none, as in
        predict(x, 'full', leave_out=...).  ``log``: log(out + 1e-12), for soft labels.  Honours set_support_weights (as a
        constant; learnable weights are read detached) and return_mask.  Inference only.  A sharded bank, a missing bank,
        a custom kernel module and a bank without values are refused (NWHipError)."""
        self._served("predict_values", early_only=True)
        if getattr(self, 'support_values', None) is None:
            raise ops.NWHipError(f"{WHAT['predict_values']}: no values are set for the bank: call set_support_values "
                                 "(precompute() clears them)")
        return self._result(self._values_head(self._eval_featurizer()(x).detach(), leave_out, log, "predict_values"))

    def forward_values(self, x, leave_out=None, log=False, weights_grad=False):
        """Not in the reference: the VALUE head at TRAINING time, the twin of predict_values as forward_bank is of predict --
        (B, T) fp32 estimates of ``self.featurizer(x)`` over precompute()'s bank and the value rows of set_support_values,
        differentiable in the featurizer, the projection and a clip scale (ops.nw_head_values_bank: the query gradient is
        computed without a (B, N) matrix; a full_precision="fp16" bank or one whose labels are not class-sorted goes
        through the score matrix).  The featurizer is taken as it is, not the folded eval copy.  ``leave_out``: (B,) int64,
        the bank row of each query or -1 for none (a leave-one-out regression loss over the bank's own samples).  ``log``:
        log(out + 1e-12), for soft labels under a KL or cross-entropy loss.  Honours return_mask.

        The bank and the values are CONSTANTS here (unless made learnable, below), as in forward_bank: ``bank_features``
        keeps the batch's features,
        detached, for refresh_bank(rows).  Support weights (set_support_weights) are honoured as a constant; LEARNABLE
        weights are read detached -- no gradient reaches ``support_logw`` from this head.  Value columns with a large
        common offset lose that many bits of the gradient (ops.nw_head_values_bank): centre them.  A sharded bank, a missing
        bank, a custom kernel module and a bank without values are refused (NWHipError), like predict_values.

        LEARNABLE values (set_support_values(..., learnable=True)) are passed with their graph: a loss on the output puts a
        gradient on ``support_targets``.  ``weights_grad=True`` passes learnable support weights with their graph as well,
        so that ``support_logw`` learns from this head too; the default keeps the detached read described above.  Both go
        through ops.nw_head_values_bank(support_grad=True) (no (B, N) matrix).

        LEARNABLE BANK ROWS: after set_bank_learnable() the parameter ``support_bank`` is passed with its graph, as
        forward_bank does, and a loss on the output puts a gradient on it (no (B, N) matrix on the fused route;
        the matrix composition elsewhere) -- with ``leave_out``, and beside learnable ``support_targets`` and
        ``weights_grad=True``.  After an optimizer step on the rows the next call re-prepares the bank in place."""
        what = WHAT["forward_values"]
        self._served("forward_values", early_only=True)    # (a sharded or missing bank: no featurizer pass)
        vals = self._values()
        if vals is None:
            raise ops.NWHipError(f"{what}: no values are set for the bank: call set_support_values (precompute() clears them)")
        qfeat = self.featurizer(x)
        self.bank_features = qfeat.detach()
        sfeat, _sy, cache = self._resident_bank("forward_values", qfeat.device)
        window = None if leave_out is None else self._leave_out_window(leave_out, qfeat, what)
        rows = self._parameters.get('support_bank')     # learnable rows: the parameter with its graph
        learn = weights_grad or rows is not None or self._parameters.get('support_targets') is not None
        support = {"support_grad": True} if learn else {}
        out = ops.nw_head_values_bank(qfeat, sfeat if rows is None else rows, cache, vals, self.kernel.kind,
                                      self.kernel._logit_scale(), row_window=window, exclude=window is not None,
                                      row_logw=self._weights(graph=bool(weights_grad)), log=log, **support)
        return self._result(out)

    def predict_loo_values(self, rows=None, batch_size=256, log=False):
        """Not in the reference: leave-one-out value estimates of the bank's own rows, (len(rows), T) -- row i's value
        predicted from every row but itself (LOO regression error, bandwidth / kernel selection, screening of noisy
        targets), mirroring predict_loo: the queries are full_feat[rows], no featurizer pass, batches of ``batch_size``,
        the exclusion inside the kernel before the softmax.  ``rows``: (R,) int64 bank rows, default all.  Honours
        set_support_weights, return_mask and ``log`` like predict_values; refuses what it refuses."""
        self._served("predict_loo_values", early_only=True)
        vals = self._values()
        if vals is None:
            raise ops.NWHipError(f"{WHAT['predict_loo_values']}: no values are set for the bank: call set_support_values "
                                 "(precompute() clears them)")
        dev = self.full_feat.device
        rows = torch.arange(self.full_feat.shape[0], device=dev) if rows is None else torch.as_tensor(rows, device=dev)
        outs = [self._values_head(self.full_feat[r], r, log, 'predict_loo_values') for r in rows.split(max(int(batch_size), 1))]
        return self._result(torch.cat(outs) if outs else torch.empty(0, vals.T, device=dev))

    def predict(self, x, mode='random', leave_out=None):
        """leave_out (not in the reference; mode='full' over precompute()'s bank only): (B,) int64, the bank row of each
        query or -1 for none -- query b is predicted without that row (see predict_loo).  Any other mode or a sharded bank:
        NWHipError."""
        if leave_out is not None:
            self._served("predict", early_only=True, mode=mode, leave_out=True)    # (another mode, a sharded or missing bank)
            return self._result(self._predict_leave_out(self._eval_featurizer()(x).detach(), leave_out, "predict_leave_out"))
        qfeat = self._eval_featurizer()(x)
        if self._served("predict", mode=mode) == "sharded":
            bank = self.sharded_bank
            return self._result(bank.predict(qfeat.detach()) if mode == 'full' else bank.predict_knn(qfeat.detach(), self.n_neighbors))
        sfeat, sy = self.support_eval.get_support(mode, x=qfeat)
        if self.debug_mode:
            print('qx shape:', x.shape)
            print('sfeat shape:', [f.shape for f in sfeat] if mode == 'ensemble' else sfeat.shape)
            print('sy:', sy)
        if mode == 'ensemble':
            probs = sum(self.nwhead(qfeat, f.to(x.device), y.to(x.device)).exp() for f, y in zip(sfeat, sy))
            out = torch.log(probs / len(sfeat))
        elif mode == 'full':
            sfeat, sy, cache = self._resident_bank(device=x.device, rows=(sfeat, sy))
            w = self._weights()
            if w is not None:    # (set_support_weights: a built-in score kernel)
                out = ops.nw_head_bank(qfeat, sfeat, sy, self.n_classes, cache, self.kernel.kind, self.kernel._logit_scale(), row_logw=w)
            else:
                out = self.nwhead(qfeat, sfeat, sy, support_cache=cache)
        else:
            out = self.nwhead(qfeat, sfeat.to(x.device), sy.to(x.device))
        return self._result(out)

    def get_neighbors(self, x, k=None):
        """Support indices ordered from nearest to farthest under the configured kernel.  k (not in the reference): only the
        k nearest, (B, k), 1 <= k <= N -- for k <= 32 over precompute()'s bank (N % 4 == 0) without the (B, N) score matrix
        where that pays (ops.nw_knn, ops.knn_fused_pays).  After precompute_sharded() (and no precompute()): the k <= 32
        nearest rows of the whole sharded bank, global rows in precompute()'s row order, the same on every rank; k is
        required there.
        NWNet(search_precision="fp16"): for k <= 32 the exact search over the fp16-rounded features of the half-precision
        bank (ops.nw_knn(rounded=True)) whenever the bank can serve it, at every size; k > 32 or k=None falls back to the
        routes above."""
        qfeat = self._eval_featurizer()(x).detach()
        if self._served("get_neighbors", k_given=k is not None) == "sharded":
            return self.sharded_bank.neighbors(qfeat, k)
        N = self.full_feat.shape[0]
        if k is not None:
            k = int(k)
            if not 1 <= k <= N:
                raise ops.NWHipError(f"get_neighbors: k = {k} outside [1, N = {N}]")
            if isinstance(self.kernel, _ScoreModule):
                sfeat, _sy, bank = self._resident_bank(rebuild=False)
                idx = routed_search(qfeat, bank, sfeat, k, self.kernel.kind, self.kernel._logit_scale(), self.search_precision)
                if idx is not None:
                    return idx
        # (a custom kernel module, k=None, or the gates of the routed search keep it: the scores, ranked whole)
        scores = self.kernel(qfeat, self.full_feat.to(qfeat.device))
        order = torch.argsort(scores, dim=-1, descending=True)
        return order if k is None else order[:, :k]

    def explain(self, x, y, k=None):
        """Not in the reference (its util/metric.py:23-50 gives the influence of EVERY support, one query at a time): the k
        most helpful and the k most harmful supports of every query under the labels `y`, with their influences, over
        precompute()'s bank -- ops.nw_top_influence of the featurised queries over full_feat / full_y with the configured
        kernel, no (B, N) matrix.  k defaults to n_neighbors (1 <= k <= 32).  Rows are rows of full_feat.  A sharded bank
        (precompute_sharded() without precompute()) is not served: NWHipError."""
        self._served("explain")
        qfeat = self._eval_featurizer()(x).detach()
        sfeat, sy, bank = self._resident_bank(rebuild=False)
        return ops.nw_top_influence(qfeat, sfeat, sy, self.n_classes, y.to(qfeat.device),
                                    self.n_neighbors if k is None else int(k), self.kernel.kind, self.kernel._logit_scale(),
                                    support_cache=bank)

    # ------------------------------------------------------------------ training step
    def forward(self, x, y, metadata=None, support_data=None):
        sx, sy, sm = support_data if support_data is not None else self.support_train.get_support(y)
        if sm is None:
            sm = torch.zeros_like(sy)
        sx, sy, sm = sx.to(x.device), sy.to(x.device), sm.to(x.device)
        nq = len(x)
        feats = self.featurizer(torch.cat((x, sx), dim=0))   # joint pass: BN statistics are shared
        qfeat, sfeat = feats[:nq], feats[nq:]
        isin = torch.isin(y, sy)
        if self.debug_mode:
            print('qx shape:', x.shape, 'sx shape:', sx.shape)
            print('qfeat shape:', qfeat.shape, 'sfeat shape:', sfeat.shape)
            print('qy:', y, 'sy:', sy, 'qy in sy:', isin)
            print(f'Percent query dropped: {(1.0 - isin.float().mean().item())*100}%')
            if metadata is not None:
                print('qmeta:', metadata, 'smeta:', sm)
        out = self.nwhead(qfeat, sfeat, sy)
        return (out, isin) if self.return_mask else out
