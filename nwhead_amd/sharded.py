"""'full' inference against a support bank sharded over the ranks of one node.

Rank g owns a contiguous slice of the (class-sorted) bank.  Queries are replicated; each rank runs
the partial forward over its slice (HIP), the ranks exchange ONE packed buffer per bucket of query
batches -- [m | den | num] per batch -- with a single RCCL all-gather over xGMI (payloads are a few
hundred KB: latency-bound, so batches are bucketed and the collective of bucket i overlaps the
kernels of bucket i+1), and every rank merges to the same (B,C) log-probabilities.

The neighbour modes go the same way: every rank searches its slice for each query's k best rows (ops.nw_knn), the ranks
exchange one packed buffer [vals | rows | labels] of 3 B k words, and every rank merges the G sorted lists to the k best
overall and, for 'knn' / 'hnsw' prediction, evaluates the head of each query's own k neighbours (ops.nw_knn_merge).

    one process per GPU, torch.distributed backend "nccl" (= RCCL on ROCm); "gloo" in CPU tests,
    where the compute hooks are replaced by the oracle (tests/test_sharded_gloo.py).
"""
from __future__ import annotations

import torch
import torch.distributed as dist

from . import ops
from ._lib import NWHipError


def shard_bounds(n_rows: int, world: int, rank: int):
    """Contiguous, near-equal split: rows [lo, hi) of the bank belong to `rank`."""
    base, extra = divmod(n_rows, world)
    lo = rank * base + min(rank, extra)
    return lo, lo + base + (1 if rank < extra else 0)


def _coalesce(chunk):
    """One (nb*B, d) tensor for a bucket of (B, d) query batches: a VIEW when the batches already sit back to
    back in one storage (slices of a staging buffer, the usual case in a serving loop), else a copy."""
    first = chunk[0]
    if first.is_contiguous() and first.dim() == 2:
        base = first.untyped_storage().data_ptr()
        step = first.numel() * first.element_size()
        if all(c.dtype == first.dtype and c.shape == first.shape and c.is_contiguous() and
               c.untyped_storage().data_ptr() == base and c.data_ptr() == first.data_ptr() + k * step
               for k, c in enumerate(chunk)):
            return first.as_strided((len(chunk) * first.shape[0], first.shape[1]), (first.shape[1], 1))
    return torch.cat(chunk, dim=0)


class ShardedBank:
    def __init__(self, feat_shard, y_shard, n_classes, kind="euclidean", logit_scale=None, group=None,
                 partial_fn=None, merge_fn=None, persistent_wgs=None, precision="fp32", row_lo=None, search_fn=None,
                 knn_merge_fn=None, search_precision="fp32"):
        """row_lo: the global bank row of this shard's first row (what neighbors() adds to the shard's own row numbers).
        Default: the exclusive prefix sum of the shard sizes over the ranks, from the all-gather below.
        search_fn / knn_merge_fn: CPU compute hooks of the neighbour search, like partial_fn / merge_fn:
        search_fn(q, k) -> (rows (B,k) int64 of THIS shard, scores (B,k) fp32), best first, equal scores by ascending row;
        knn_merge_fn(vals, rows, labels, k, n_classes) -> what ops.nw_knn_merge returns.
        The neighbour search runs on the fp32 shard through a SplitBank of split-fp16 rows (fp32-grade scores): with
        precision="fp32" that is the bank 'full' inference uses; with precision="fp16" a second bank is prepared from the
        fp32 shard on the first search (the fp16-packed rows are not searched), so 'full'-only users pay nothing.
        search_precision="fp16" (needs precision="fp16"): the search runs on the shard's fp16 bank itself
        (ops.nw_knn(rounded=True): the exact search over the fp16-rounded features), no second bank is ever prepared, and
        predict_knn is the k-NN head of the rounded scores.  (A shard of 25 rows or fewer, whose bank holds norms only, is
        searched through its score matrix: fp32 scores of the unrounded rows.)
        precision: "fp32" (split-fp16 rows, fp32-grade) or "fp16" (the reduced-precision bank of ops.SplitBank).
        persistent_wgs: workgroups of the persistent tile kernel (nw_fwd_opts.persistent_wgs, a multiple of 8; 0 = one per
        CU).  Default: with more than one rank, all CUs but one per XCD (count - 8) -- the all-gather of bucket i runs
        under the kernels of bucket i + 1, and a kernel that holds one 160 KB-LDS workgroup on EVERY CU would leave RCCL's
        kernel nowhere to run until it ends; with one rank, one per CU."""
        if search_precision not in ("fp32", "fp16"):
            raise ValueError(f"search_precision must be 'fp32' or 'fp16', got {search_precision!r}")
        if search_precision == "fp16" and precision != "fp16":
            raise ValueError("search_precision='fp16' searches the half-precision bank: it needs precision='fp16'")
        self.search_precision = search_precision
        self.feat = feat_shard.detach().to(torch.float32).contiguous()
        self.y = y_shard.detach().to(torch.int64).contiguous()
        self.C = int(n_classes)
        self.kind, self.logit_scale, self.group = kind, logit_scale, group
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        self._partial = partial_fn or self._hip_partial
        self._merge = merge_fn or self._hip_merge
        self._ws = None           # this bank's own scratch buffer (ops._partials lets it grow)
        if persistent_wgs is None:
            persistent_wgs = 0
            if self.world > 1 and self.feat.is_cuda:
                cus = torch.cuda.get_device_properties(self.feat.device).multi_processor_count
                persistent_wgs = max(8, (cus - 8) // 8 * 8)
        self.persistent_wgs = int(persistent_wgs)
        # Class windows: a contiguous slice of a class-sorted bank holds only ~C/G classes, so its
        # partial forward runs on labels shifted by the slice's lowest class with CL = widest window
        # over the ranks; the exchanged rows are (2 + CL) instead of (2 + C) floats per query.
        self.class_lo, self.CL, self.y_local = None, self.C, self.y
        self._search = search_fn or self._hip_search
        self._knn_merge = knn_merge_fn or ops.nw_knn_merge
        self._search_bank = None
        self.n_total = int(self.feat.shape[0])       # rows of the whole bank
        if self.world > 1:
            lo = int(self.y.min()) if self.y.numel() else 0
            hi = int(self.y.max()) if self.y.numel() else -1
            box = torch.tensor([lo, hi, self.feat.shape[0]], dtype=torch.int64, device=self.feat.device)
            allb = torch.empty(self.world, 3, dtype=torch.int64, device=self.feat.device)
            dist.all_gather_into_tensor(allb.view(-1), box, group=group)
            sizes = allb[:, 2].tolist()
            self.n_total = int(sum(sizes))
            if row_lo is None:
                row_lo = sum(sizes[:dist.get_rank(group)])
            width = int((allb[:, 1] - allb[:, 0] + 1).clamp_min(1).max())
            if width < self.C:
                self.CL = width
                self.class_lo = allb[:, 0].clamp(0, max(self.C - 1, 0)).contiguous()
                self.y_local = (self.y - lo).contiguous()
        # the shard never changes: prepare it once (squared norms + split-fp16 rows, ops.SplitBank)
        self.cache = ops.SplitBank(self.feat, precision=precision) if (partial_fn is None and self.feat.is_cuda) else None
        self.norm2 = self.cache.norm2 if self.cache is not None else None
        if self.cache is not None and self.cache.has_operand_rows:
            self.cache.build_tables(self.y_local)   # the labels every call of this shard passes (self.y when there is one rank)
        self.row_lo = int(row_lo or 0)

    # ---- HIP compute hooks (the product path)
    def _hip_partial(self, packed_row, q):
        self._ws = ops._partials(packed_row, q, self.feat, self.y_local, self.CL, self.kind, self.logit_scale, ws=self._ws,
                                 cache=self.cache, persistent_wgs=self.persistent_wgs, own_ws=True)

    def _hip_merge(self, gathered_rows, B):
        return ops.nw_merge(gathered_rows, B, self.C, class_lo=self.class_lo, c_local=self.CL)

    def _hip_search(self, q, k):
        # A shard picks no route: its candidates always come from nw_knn (whose order the cross-shard merge expects), and
        # nw_knn asks ops.knn_route.  What is decided here is a demand, not a route: search_precision="fp16" over packed rows
        # passes rounded=True, so that a search the rounded route refuses (queries that do not pad to the shard's width)
        # raises nw_knn's refusal where KNN.indices and get_neighbors fall back.  A norms-only fp16 shard (25 rows or fewer)
        # has nothing to round and is searched like any other bank.
        half = self.search_precision == "fp16" and self.cache is not None
        if half and self.cache.packed is not None:
            return ops.nw_knn(q, self.cache, k, self.kind, self.logit_scale, return_values=True, rounded=True,
                              persistent_wgs=self.persistent_wgs)
        bank = self.cache if half else self._search_bank
        if bank is None:
            # (the 'full' bank has split rows and no class-sorted copy -- it was prepared without labels -- unless it is fp16)
            bank = self.cache if (self.cache is not None and self.cache.precision == "fp32") else ops.SplitBank(self.feat)
            self._search_bank = bank
        return ops.nw_knn(q, bank, k, self.kind, self.logit_scale, return_values=True, support=self.feat)

    # ---- neighbour search
    def knn_partial(self, q, k):
        """This rank's packed candidates for one (B,d) query batch: a flat int32 buffer [vals | rows | labels] of 3 B k
        words -- per query the min(k, shard rows) best rows of the shard, best first, as (score bits, GLOBAL bank row,
        GLOBAL class id), padded to k with no-element slots (-inf, -1, -1).  An empty shard emits only those."""
        k = int(k)
        q = q.detach().to(torch.float32).contiguous()
        B, n = q.shape[0], self.feat.shape[0]
        kk = min(k, n)
        buf = torch.empty(3, B, k, dtype=torch.int32, device=self.feat.device)
        vals = buf[0].view(torch.float32)
        if kk < k:
            vals.fill_(float("-inf"))
            buf[1:].fill_(-1)
        if kk > 0 and B > 0:
            idx, val = self._search(q, kk)
            vals[:, :kk] = val
            buf[1, :, :kk] = idx + self.row_lo
            buf[2, :, :kk] = self.y[idx]
        return buf.view(-1)

    def _knn(self, q, k, n_classes):
        k = int(k)
        if k > ops.KNN_MERGE_MAX_K:
            raise NWHipError(f"ShardedBank: k = {k} neighbours; the cross-shard merge takes at most {ops.KNN_MERGE_MAX_K}")
        if k < 1 or k > self.n_total:
            raise NWHipError(f"ShardedBank: k = {k} outside [1, N = {self.n_total}] (the rows of the whole bank)")
        if self.world > ops.KNN_MERGE_MAX_SHARDS or self.n_total >= 2 ** 31:
            raise NWHipError(f"ShardedBank: the cross-shard merge takes at most {ops.KNN_MERGE_MAX_SHARDS} shards and "
                             f"2^31 - 1 bank rows, got {self.world} and {self.n_total}")
        B, G = q.shape[0], self.world
        packed = self.knn_partial(q, k)
        if G > 1:
            gathered = torch.empty(G, packed.numel(), dtype=torch.int32, device=packed.device)
            dist.all_gather_into_tensor(gathered.view(-1), packed, group=self.group)
        else:
            gathered = packed.view(1, -1)
        n = B * k
        vals, rows, labels = (gathered[:, i * n:(i + 1) * n].view(G, B, k) for i in range(3))   # views: the kernel strides
        return self._knn_merge(vals.view(torch.float32), rows, labels, k, n_classes)

    def neighbors(self, q, k, return_values=False, return_labels=False):
        """The k nearest rows of the WHOLE bank for every query: (B,k) int64 global rows, best score first, equal scores by
        ascending row; optionally their (B,k) scores and (B,k) int64 class ids.  One all-gather of 3 B k words (none with
        one rank); identical on every rank.  1 <= k <= min(32, bank rows)."""
        idx, vals, labels = self._knn(q, k, None)
        res = (idx,) + ((vals,) if return_values else ()) + ((labels,) if return_labels else ())
        return res if len(res) > 1 else idx

    def predict_knn(self, q, k):
        """(B,d) -> (B,C) log-probabilities of every query over its OWN k nearest supports of the whole bank -- the
        semantics of NWNet(knn_per_query=True) -- identical on every rank."""
        return self._knn(q, k, self.C)[3]

    def row_len(self, B):
        return 2 * B + B * self.CL

    def predict(self, q):
        """One query batch: (B,d) -> (B,C) log-probabilities, identical on every rank."""
        return self.predict_stream([q], bucket=1)[0]

    def predict_stream(self, batches, bucket=8):
        """Pipelined prediction of a list of (B_i, d) query batches (B_i may differ: the ragged tail of a
        loader is an ordinary case).

        Every `bucket` consecutive batches are coalesced into ONE launch of the partial forward (the
        kernel tiles over queries anyway, and one launch over the bucket's rows amortises the launch,
        the tile prologue and the merge), ONE packed buffer [m | den | num] and ONE all-gather; the
        merge of bucket i runs after the kernels of bucket i+1 have been queued, so the collective
        flies under them.  Outputs are returned per batch, in order."""
        if not batches:
            return []
        d = batches[0].shape[-1]
        for k, qb in enumerate(batches):
            if qb.dim() != 2 or qb.shape[1] != d:
                raise ValueError(f"predict_stream: batch {k} has shape {tuple(qb.shape)}, expected (B, {d})")
        dev, G = self.feat.device, self.world
        outs, pending = [], None
        ring = {}

        def split(out, sizes):
            pos = 0
            for n in sizes:
                outs.append(out[pos:pos + n])
                pos += n

        def finish(p):
            work, gathered, sizes = p
            if work is not None:
                work.wait()
            split(self._merge(gathered, sum(sizes)), sizes)          # (rows of the bucket, C)

        for n_bucket, i0 in enumerate(range(0, len(batches), bucket)):
            chunk = batches[i0:i0 + bucket]
            sizes = [int(c.shape[0]) for c in chunk]
            Bq = sum(sizes)
            L = self.row_len(Bq)
            key = (n_bucket % 3, Bq)
            if key not in ring:
                ring[key] = (torch.empty(L, dtype=torch.float32, device=dev),
                             torch.empty(G, L, dtype=torch.float32, device=dev))
            packed, gathered = ring[key]
            qcat = chunk[0] if len(chunk) == 1 else _coalesce(chunk)
            if G == 1 and self._partial == self._hip_partial:
                # one rank: nothing to exchange, the forward finalises in place
                split(ops.nw_head(qcat, self.feat, self.y, self.C, self.kind, self.logit_scale, support_cache=self.cache),
                      sizes)
                continue
            self._partial(packed, qcat.detach().to(torch.float32).contiguous())
            if G > 1:
                work = dist.all_gather_into_tensor(gathered.view(-1), packed, group=self.group, async_op=True)
            else:
                gathered, work = packed.view(1, L), None
            if pending is not None:
                finish(pending)
            pending = (work, gathered, sizes)
        if pending is not None:
            finish(pending)
        return outs
