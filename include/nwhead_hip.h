/*
 * nwhead_hip.h -- C ABI of libnwhead_hip.so: the MI355X (gfx950) implementation of the
 * Nadaraya-Watson head hot path of alanqrwang/nwhead @ 2024_08_07.
 *
 * The reference has no FFI; its seam is the Python operator
 *     NWHead.forward(x, sx, sy)            nwhead/nw.py:266-289
 * built from                               nwhead/kernel.py:13-44   (score functions)
 * plus util/metric.py:23-50 (support_influence) and the implicit autograd of the above
 * (loss.backward(), train.py:414).  Each entry point below names the reference lines it
 * replaces.  INTEGRATION.md shows the ctypes binding a reference maintainer would add.
 *
 * Conventions (all entry points):
 *   - every pointer is a DEVICE pointer into HIP memory owned by the caller, row-major, dense;
 *     float = IEEE fp32, labels = int64 (torch.long), sizes = int64;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); calls only enqueue
 *     work on it: they never synchronise, never allocate, never free;
 *   - return value: NW_OK (0) or a negative nw_status; nothing is thrown;
 *   - stateless and thread-safe: safe from any host thread with its own stream; every option of a call is an argument
 *     of that call (nw_fwd_opts), and the library never reads the process environment.  The one piece of process state is
 *     the table of diagnostic knobs (nw_debug_set, nw_debug_tile_timing): timing experiments, unset in normal use;
 *   - scratch memory is supplied by the caller; ask nw_*_workspace_bytes() for the size.
 */
#ifndef NWHEAD_HIP_H
#define NWHEAD_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NW_ABI_VERSION 2

/* score functions = the reference's kernel modules, nwhead/kernel.py:80-97 (get_kernel) */
typedef enum {
    NW_SCORE_EUCLIDEAN = 0,   /* -cdist(x, y)                           kernel.py:13-15 */
    NW_SCORE_HYPERSPHERE = 1, /* -cdist(normalize(x), normalize(y))     kernel.py:17-21 */
    NW_SCORE_COSINE = 2,      /* normalize(x) . normalize(y)            kernel.py:23-28 */
    NW_SCORE_DOT = 3,         /* x . y                                  kernel.py:30-33 */
    NW_SCORE_CLIP = 4         /* exp(logit_scale) * cosine              kernel.py:35-44 */
} nw_score_kind;

typedef enum {
    NW_OK = 0,
    NW_ERR_INVALID_ARG = -1,  /* null pointer, negative size, label array missing ...          */
    NW_ERR_UNSUPPORTED = -2,  /* unknown score kind                                             */
    NW_ERR_WORKSPACE = -3,    /* workspace smaller than nw_*_workspace_bytes()                  */
    NW_ERR_LAUNCH = -4,       /* hipLaunchKernel / hipMemsetAsync reported an error             */
    NW_ERR_NO_DEVICE = -5     /* no gfx950 device visible to this process                       */
} nw_status;

int nw_abi_version(void);
const char *nw_status_string(int status);
/* 0 when a HIP device is visible and its arch is gfx950, else NW_ERR_NO_DEVICE. */
int nw_device_check(void);

/* ---------------------------------------------------------------------------------------------
 * Scores only.  Replaces kernel(x, y): nwhead/kernel.py:13-44 as called from nwhead/nw.py:283
 * (x unsqueezed to (B,1,d), y = support) and from NWNet.get_neighbors nwhead/nw.py:248 and
 * KNN.__call__ nwhead/utils.py:187 (2-D queries x bank).
 *   q        (B,d)
 *   s        (N,d) when sup_batched == 0, (B,N,d) when sup_batched != 0
 *   scores   (B,N) out
 *   logit_scale_dev  device pointer to the CLIP log-scale scalar (kernel.py:38); only read for
 *                    NW_SCORE_CLIP; may be NULL otherwise
 * cdist regime (torch picks the matmul form when N > 25, else the direct difference form): the
 * same switch is made here so that exact-zero distances behave as in the reference.
 * ------------------------------------------------------------------------------------------- */
int nw_scores_f32(const float *q, const float *s, float *scores,
                  int64_t B, int64_t N, int64_t d,
                  int kind, const float *logit_scale_dev, int sup_batched, void *stream);

/* Squared L2 norm of every row of a dense (rows,d) matrix: n2[r] = sum_k x[r,k]^2.  The pow(2).sum(-1)
 * half of torch.cdist's matmul form (and of F.normalize, nwhead/kernel.py:19-20), hoisted out of the
 * hot loop for operands that do not change between calls (the precomputed support bank). */
int nw_row_norm2_f32(const float *x, float *n2, int64_t rows, int64_t d, void *stream);

/* Split-fp16 form of a dense (rows,d) fp32 matrix, d % 32 == 0 (NW_ERR_UNSUPPORTED otherwise):
 *   out_split (rows,d) floats-worth of bytes: every 128-byte chunk of a row = [32 x h | 32 x l] fp16 with
 *             h + l = x * 2^e to 2^-23 relative, e per row such that the row's largest magnitude lands
 *             in [2^13, 2^14) (fp16 normal range whatever the feature scale);
 *   row_scale (rows,) = 2^-e;   row_norm2 (rows,) = sum_k x_k^2 of the original values.
 * Like nw_row_norm2_f32 this belongs to precompute() (nwhead/nw.py:118-125): the bank is split once. */
int nw_split_rows_f16x2(const float *x, float *out_split, float *row_scale, float *row_norm2,
                        int64_t rows, int64_t d, void *stream);

/* Half-precision form of a dense (rows,d) fp32 matrix, d % 64 == 0 (NW_ERR_UNSUPPORTED otherwise): the operand of
 * nw_fwd_opts.operand_form = 1.  The scale rule is nw_split_rows_f16x2's (e = 14 - frexp exponent of the row's largest
 * magnitude, at most 126; 0 for an all-zero row or a non-finite maximum), but only the rounded value is kept:
 *   out_rows  (rows,d) fp16, dense, row-major: h = fp16(x * 2^e), round to nearest even;
 *   row_scale (rows,) = 2^-e;   row_norm2 (rows,) = sum_k (h_k * 2^-e)^2 in fp32: the norms of the ROUNDED rows.
 * Half the bytes of the split form and one fp16 product per term instead of three; the head computed from these
 * operands is the exact head of the rounded features h * 2^-e (relative rounding 2^-11 per element). */
int nw_pack_rows_f16(const float *x, uint16_t *out_rows, float *row_scale, float *row_norm2,
                     int64_t rows, int64_t d, void *stream);

/* Rows of a PREPARED bank replaced in place: R given rows of the fp32 matrix get new values and every prepared form
 * of those rows is left, bit for bit, as the three calls above would have made it from the new fp32 row.  For a
 * memory bank that follows the weights during training (each batch's features written back, optionally blended with
 * what was there) and for swapping samples of a live bank; the labels do not change.
 *   x        (R, dx) fp32, 1 <= dx <= d; columns dx .. d-1 of a new row are zero (the bank's zero padding).  Any
 *            alignment and width (16-byte loads only when dx % 4 == 0 and x is 16-byte aligned)
 *   rows     (R,) int64 on the device
 *   momentum 0: the new row is x[i], its bits as they are (-0 and NaN pass unchanged); otherwise
 *            momentum * old + (1.0f - momentum) * x[i] with the two products and the sum each rounded on their own,
 *            old read from s_rows, 1.0f - momentum formed in fp32
 *   s_rows   (N, d) fp32: the matrix the prepared forms are derived from (read for the blend, written)
 *   s_user   optional (N, dx): the caller's own tensor when s_rows is a zero-padded copy of it; receives the first
 *            dx columns of the new row
 *   s_norm2  (N,)
 *   s_split + s_scale               optional as a group: the forms of nw_split_rows_f16x2 (s_norm2 is then its
 *            row_norm2; the "split_lbits" diagnostic knob applies as it does there)
 *   s_f16 + f16_scale + f16_norm2   optional as a group: the forms of nw_pack_rows_f16.  With this group alone
 *            s_norm2 is nw_row_norm2_f32's
 * Item i with r = rows[i] is skipped when r < 0, when r >= N (compared, never used as an address) or when a later
 * item j > i names the same row: the LAST occurrence wins, the others take no part, not even in the blend.  Whatever
 * a skipped item would touch, and every row no item names, keeps its bits.
 * One launch, one wave per item: no workspace, no allocation, no synchronisation, no environment, no atomics.
 * Status, decided in this order before anything is launched: a negative size, dx outside [1, d], a momentum that is
 * not finite or outside [0, 1): NW_ERR_INVALID_ARG;  R == 0 or N == 0: NW_OK;  x, rows, s_rows or s_norm2 NULL, a
 * form group given in part, s_rows / s_split / s_f16 not 16-byte aligned: NW_ERR_INVALID_ARG;  neither form group
 * (a norms-only bank), the split group with d % 32 != 0, the fp16 group with d % 64 != 0 or d < 192, R > 16384 (every
 * wave scans the rest of `rows` for its row): NW_ERR_UNSUPPORTED. */
int nw_bank_update_rows_f32(const float *x, const int64_t *rows, int64_t R, int64_t dx, float momentum,
                            float *s_rows, float *s_user, float *s_norm2,
                            float *s_split, float *s_scale,
                            void *s_f16, float *f16_scale, float *f16_norm2,
                            int64_t N, int64_t d, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Forward.  Replaces NWHead.forward nwhead/nw.py:266-289:
 *     one_hot(sy) -> kernel scores -> softmax over supports -> bmm with one-hot -> log(. + 1e-12)
 *   sy          (N,) or, when labels_batched != 0, (B,N); values outside [0,C) contribute nothing
 *   s_norm2     optional (N,): squared row norms of s as written by nw_row_norm2_f32.  The resident
 *               bank of 'full' inference (NWNet.precompute, nwhead/nw.py:118-125) caches them so
 *               that the hot loop is matrix-core work only; NULL = computed inside the kernel.
 *               Only read for a shared 2-D support.
 *   s_split, s_scale   optional, d % 32 == 0 only: the support in split-fp16 form as written by
 *               nw_split_rows_f16x2 (with s_norm2 from the same call).  Selects the fast path of
 *               'full' inference: dot products on the fp16 matrix cores at fp32-grade accuracy
 *               (x = h + l, three fp16 MFMAs per product block; error ~1e-7 * sum|a_k b_k|, the
 *               level of an fp32 FMA chain).  The queries are split inside the call.  NULL = fp32
 *               matrix cores on the original operands.
 *   out         (B,C) log-probabilities
 *   scores_out  optional (B,N): raw scores (saved for backward / neighbour search)
 *   lse_out     optional (B,):  log sum_j exp(score_bj)  (saved for backward)
 *   weights_out optional (B,N): softmax weights  (the `sweights` of util/metric.py:23)
 *   workspace   nw_fwd_workspace_bytes(B,N,d,C) bytes of scratch (may be NULL if that is 0)
 * ------------------------------------------------------------------------------------------- */
/* Options of one forward call (NULL = all defaults).  struct_size = sizeof(nw_fwd_opts) of the caller's header.
 *   tables / tables_bytes  run tables of a RESIDENT bank (labels that do not change between calls), built once with
 *               nw_bank_tables_build(sy, N, C, ...) for the very sy, N and C of this call: on large launches the forward
 *               walks the bank in tiles of 128 supports and needs, per tile, the runs of equal consecutive labels; without
 *               tables it builds them in its workspace on every call (~5 us + a kernel boundary)
 *   tables_sy / tables_N   the label array and row count the tables were built from.  The forward uses the tables only
 *               when these are the call's own sy and N (anything else -- another label array, a shorter struct of an older
 *               header -- and it builds the tables itself, as without the option)
 *   persistent_wgs  workgroups of the persistent tile kernel, a multiple of 8; 0 = one per CU.  Sharded inference passes
 *               CUs - 8 (one CU per XCD left to the concurrent RCCL kernel)
 *   force_split nonzero: the split-fp16 path whenever the bank is prepared, also below ~2e8 multiply-adds
 *   operand_form (the field older headers call `reserved`; same offset, same struct size)
 *               0  s_split holds split rows (nw_split_rows_f16x2), as described above;
 *               1  s_split holds the half-precision rows of nw_pack_rows_f16, s_scale and s_norm2 come from the same
 *                  call (all three required): the optional reduced-precision head of 'full' inference.  The queries are
 *                  rounded the same way inside the call, and the result is the head of the ROUNDED queries and supports
 *                  at the accuracy of the split path -- two fp16 MFMAs per 64 terms instead of three per 32, at every
 *                  size, on the 256-query persistent kernel.  Honoured by nw_fwd_f32 (out, lse_out) and
 *                  nw_fwd_partial_f32; NW_ERR_UNSUPPORTED, before anything is launched, for scores_out / weights_out,
 *                  batched supports or labels, d % 64 != 0, d < 192, a shape the tile kernels do not take (N <= 25;
 *                  nw_fwd_workspace_bytes covers every other one) and for nw_fwd_influence_f32
 *               any other value: NW_ERR_INVALID_ARG */
typedef struct nw_fwd_opts {
    uint32_t struct_size;
    int32_t persistent_wgs;
    int32_t force_split;
    int32_t operand_form;
    const void *tables;
    size_t tables_bytes;
    const int64_t *tables_sy;
    int64_t tables_N;
} nw_fwd_opts;

size_t nw_fwd_workspace_bytes(int64_t B, int64_t N, int64_t d, int64_t C);
int nw_fwd_f32(const float *q, const float *s, const int64_t *sy, const float *s_norm2,
               const float *s_split, const float *s_scale,
               float *out, float *scores_out, float *lse_out, float *weights_out,
               void *workspace, size_t workspace_bytes,
               int64_t B, int64_t N, int64_t d, int64_t C,
               int kind, const float *logit_scale_dev,
               int sup_batched, int labels_batched, const nw_fwd_opts *opts, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Sharded 'full' inference (new capability): per-shard partials of the same
 * forward over this rank's slice of the support bank, and the merge.
 *   m    (B,)   max_j score            (-inf for an empty shard)
 *   den  (B,)   sum_j exp(score - m)
 *   num  (B,C)  sum_{j: sy_j = c} exp(score - m)
 * nw_merge_finalize_f32 takes the partials of G shards and writes
 *   out = log(num / den + 1e-12) after rescaling every shard to the common max.
 *   Shard g's arrays start at m + g*stride_m, den + g*stride_den, num + g*stride_num (strides in
 *   floats; pass B, B, B*C for dense (G,B) (G,B) (G,B,C) stacks, or the common row length when the
 *   three sections of each shard are packed in one all-gathered buffer).
 *   class_lo (device, (G,)) / C_local: optional class windows.  A contiguous slice of a class-sorted
 *   bank only holds the classes [class_lo[g], class_lo[g] + C_local); its partial forward is then run
 *   with labels shifted by class_lo[g] and C = C_local, num is (B, C_local) per shard, and the rows
 *   that cross xGMI shrink ~G-fold.  NULL = every shard carries all C classes.
 * ------------------------------------------------------------------------------------------- */
int nw_fwd_partial_f32(const float *q, const float *s, const int64_t *sy, const float *s_norm2,
                       const float *s_split, const float *s_scale,
                       float *m, float *den, float *num,
                       void *workspace, size_t workspace_bytes,
                       int64_t B, int64_t N, int64_t d, int64_t C,
                       int kind, const float *logit_scale_dev, const nw_fwd_opts *opts, void *stream);
int nw_merge_finalize_f32(const float *m, const float *den, const float *num, float *out,
                          int64_t G, int64_t B, int64_t C,
                          int64_t stride_m, int64_t stride_den, int64_t stride_num,
                          const int64_t *class_lo, int64_t C_local, void *stream);

/* Run tables of a RESIDENT bank for nw_fwd_opts.tables:
 *     tables = malloc(nw_bank_tables_bytes(N));  nw_bank_tables_build(sy, N, C, tables, bytes, stream);   (once)
 *     opts.tables = tables; opts.tables_bytes = bytes;  nw_fwd_f32(..., &opts, stream)                     (per call)
 * Labels outside [0, C) are kept out of the tables like everywhere else (they contribute nothing). */
size_t nw_bank_tables_bytes(int64_t N);
int nw_bank_tables_build(const int64_t *sy, int64_t N, int64_t C, void *tables, size_t tables_bytes, void *stream);


/* ---------------------------------------------------------------------------------------------
 * Backward.  Replaces the autograd graph the reference builds through nwhead/nw.py:276-289 and
 * nwhead/kernel.py:13-44 (loss.backward(), train.py:414), including torch's zero sub-gradient at
 * distance 0 (_euclidean_dist_backward / cdist_backward mask).
 *   scores, lse   as saved by nw_fwd_f32
 *   out, gout     (B,C) forward output and its incoming gradient
 *   gq            (B,d) out;  gs (N,d) or (B,N,d) out;  glogit_scale optional scalar out (CLIP)
 *   workspace     nw_bwd_workspace_bytes(...) bytes
 * nw_bwd_workspace_bytes and nw_bwd_uses_split are two fields of one plan (route, launch sizes, workspace map):
 * nw_debug_bwd_plan returns all of it.
 * ------------------------------------------------------------------------------------------- */
size_t nw_bwd_workspace_bytes(int64_t B, int64_t N, int64_t d, int64_t C, int kind, int sup_batched);
int nw_bwd_f32(const float *q, const float *s, const int64_t *sy,
               const float *scores, const float *lse, const float *out, const float *gout,
               float *gq, float *gs, float *glogit_scale,
               void *workspace, size_t workspace_bytes,
               int64_t B, int64_t N, int64_t d, int64_t C,
               int kind, const float *logit_scale_dev,
               int sup_batched, int labels_batched, void *stream);
/* The same with the supports' bank as prepared for the forward (nw_split_rows_f16x2 of these very rows: s_split,
 * s_scale, s_norm2; all three or none; shared (N,d) supports only).  On large shapes -- nw_bwd_uses_split(...) != 0:
 * shared supports, d % 32 == 0, a row of N coefficients fits in LDS -- the two products of the backward
 * (gq = A s + 2 rq q, gs = A^T q + 2 rs s) run on the fp16 matrix cores with split-row operands like the forward
 * (three fp16 MFMAs per fp32 multiply-add, fp32 accumulation); without a bank the rows are split inside the call.
 * A training step builds the bank once, hands it to nw_fwd_f32 (scores saved for the backward) and to this call.
 * The caller's s_split (exactly N * d floats, no tail required) is used when d % 64 == 0; for d % 64 == 32 the rows
 * are split again into the workspace, whose copy carries the tail the product kernel's last column tile reads. */
int nw_bwd_uses_split(int64_t B, int64_t N, int64_t d, int64_t C, int sup_batched);
int nw_bwd_bank_f32(const float *q, const float *s, const float *s_norm2, const float *s_split,
                    const float *s_scale, const int64_t *sy,
                    const float *scores, const float *lse, const float *out, const float *gout,
                    float *gq, float *gs, float *glogit_scale,
                    void *workspace, size_t workspace_bytes,
                    int64_t B, int64_t N, int64_t d, int64_t C,
                    int kind, const float *logit_scale_dev,
                    int sup_batched, int labels_batched, void *stream);


/* ---------------------------------------------------------------------------------------------
 * support_influence.  Replaces util/metric.py:23-50, vectorised over the query batch:
 *   infl[b,j] = log((p - p*w_bj) / (p - w_bj*[sy_j == qy_b])),  p = probs[b, qy_b]
 *   probs (B,C) = exp(out);  qy (B,) int64;  w (B,N) softmax weights;  sy (N,) int64
 * Every product/difference/quotient is rounded separately (no FMA contraction) so the +inf / NaN
 * pattern of the reference's one-shot classes is reproduced.
 * ------------------------------------------------------------------------------------------- */
int nw_support_influence_f32(const float *probs, const int64_t *qy, const float *w,
                             const int64_t *sy, float *infl,
                             int64_t B, int64_t N, int64_t C, void *stream);

/* Softmax over supports + label aggregation + log of a GIVEN (B,N) score matrix, and its gradient: the tail of
 * NWHead.forward (nwhead/nw.py:285-289) for score functions that are not built into the kernels (the reference
 * accepts any callable kernel module, nw.py:256-264: the scores then come from that module, on the device, through
 * torch autograd; this is the rest).  sy (N,) or (B,N) when labels_batched.
 *   nw_aggregate_f32      out (B,C), optional lse_out (B,), optional weights_out (B,N)
 *   nw_aggregate_bwd_f32  gscores (B,N) = W * (dW - sum_j W dW), dW_j = gout[b, sy_j] * exp(-out[b, sy_j]) */
int nw_aggregate_f32(const float *scores, const int64_t *sy, float *out, float *lse_out, float *weights_out,
                     int64_t B, int64_t N, int64_t C, int labels_batched, void *stream);
int nw_aggregate_bwd_f32(const float *scores, const int64_t *sy, const float *lse, const float *out, const float *gout,
                         float *gscores, int64_t B, int64_t N, int64_t C, int labels_batched, void *stream);

/* Forward + support_influence in one call: nw_fwd_f32's arguments plus
 *   qy (B,) int64 query labels, infl_out (B,N).
 * The fused tile kernel writes the raw scores into infl_out, the merge gives out (log-probabilities) and the
 * log-sum-exp, and ONE in-place pass turns scores into influences with w = exp(score - lse), p = exp(out[b, qy_b])
 * (util/metric.py:23-50 applied to the head's own outputs, README.md:101-132).  The (B,N) matrix crosses HBM three
 * times (scores out, scores in, influences out) instead of five (scores, weights written and read, influences), and
 * no softmax-weight matrix exists.  (Recomputing the scores instead of storing them would cost a second pass of the
 * tile kernel: 13 us against the 4 us of the round trip at B = 256, N = 10000.)  Shared 2-D supports only.
 * lse_out optional (B,).  workspace: nw_fwd_workspace_bytes(B,N,d,C). */
int nw_fwd_influence_f32(const float *q, const float *s, const int64_t *sy, const float *s_norm2,
                         const float *s_split, const float *s_scale, const int64_t *qy,
                         float *out, float *lse_out, float *infl_out,
                         void *workspace, size_t workspace_bytes,
                         int64_t B, int64_t N, int64_t d, int64_t C,
                         int kind, const float *logit_scale_dev, const nw_fwd_opts *opts, void *stream);

/* ---------------------------------------------------------------------------------------------
 * The k best supports per query.  Replaces the full descending argsort that the reference cuts to
 * its first k columns (KNN.__call__, nwhead/utils.py:185-193; 'knn' / 'hnsw' support modes):
 *   idx_out[b][0..k) = argsort(scores[b], descending, stable)[0..k)      (ties: lower index first)
 *   scores   (B,N) fp32 (e.g. from nw_scores_f32)
 *   idx_out  (B,k) int64;  val_out optional (B,k) fp32: the selected scores, best first
 * 1 <= k <= min(N, 1024); larger k returns NW_ERR_UNSUPPORTED (callers sort the whole row then).
 * ------------------------------------------------------------------------------------------- */
int nw_topk_f32(const float *scores, int64_t *idx_out, float *val_out,
                int64_t B, int64_t N, int64_t k, void *stream);

/* ---------------------------------------------------------------------------------------------
 * The k best supports per query over a PREPARED bank, without the (B,N) score matrix.  Replaces the
 * score matrix + descending argsort + cut to k columns of the reference's neighbour modes
 * (KNN.__call__, nwhead/utils.py:185-193; NWNet.get_neighbors, nwhead/nw.py:245-249) for banks where
 * that matrix is the cost: every tile of the split-fp16 tile kernel selects its k best scores in its
 * epilogue, a second kernel takes the k best of every query's candidates.
 *   q         (B,d) fp32 queries
 *   s_split / s_scale / s_norm2   the bank as nw_split_rows_f16x2 leaves it ((N,d), (N,), (N,))
 *   idx_out   (B,k) int64 bank rows, best score first, equal scores in ascending row order
 *   val_out   optional (B,k) fp32: their scores (either zero is returned as +0.0)
 * The scores are, bit for bit, those nw_fwd_f32 writes to scores_out from the same split operands,
 * and the order is nw_topk_f32's: the result equals nw_topk_f32 of that matrix.
 * 1 <= k <= min(N, 32), d % 32 == 0, N > 25 (the tile kernels' regime); anything else returns
 * NW_ERR_UNSUPPORTED (callers go through nw_topk_f32), for which nw_knn_workspace_bytes returns 0.
 * q, s_split and workspace 16-byte aligned.  Like every entry: no allocation, no synchronisation,
 * no environment.  nw_knn_workspace_bytes is non-decreasing in B, N and k; to be so it visits the
 * smaller shapes, up to a millisecond of host time: ask once per shape and keep the answer.
 * ------------------------------------------------------------------------------------------- */
size_t nw_knn_workspace_bytes(int64_t B, int64_t N, int64_t d, int64_t k);
int nw_knn_f32(const float *q, const float *s_split, const float *s_scale, const float *s_norm2,
               int64_t *idx_out, float *val_out, void *workspace, size_t workspace_bytes,
               int64_t B, int64_t N, int64_t d, int64_t k, int kind, const float *logit_scale_dev,
               void *stream);
/* The same search restricted to a ROW WINDOW per query: row_lo / row_hi (B,) int32 on the device.  A row
 * is a candidate only when lo[b] <= row < hi[b] (exclude == 0), or only when it is outside that range
 * (exclude != 0).  lo >= hi is the empty window: no row, or with exclude every row.  The values are
 * clamped to [0, N] on the device and never used as an address.  In a class-sorted bank "the rows of
 * class c" is such a window: nearest same-class / other-class supports, leave-one-out neighbours
 * (window [i, i+1), excluded), one segment of a concatenated bank.
 * Same contract, limits, alignment rules, launch decision and workspace (nw_knn_workspace_bytes) as
 * nw_knn_f32, and the same scores bit for bit; the result is the k best rows the window admits, in
 * nw_topk_f32's order, and where it admits fewer than k the remaining slots hold row -1, value -inf.
 * row_lo or row_hi NULL: NW_ERR_INVALID_ARG. */
int nw_knn_window_f32(const float *q, const float *s_split, const float *s_scale, const float *s_norm2,
                      const int32_t *row_lo, const int32_t *row_hi, int exclude,
                      int64_t *idx_out, float *val_out, void *workspace, size_t workspace_bytes,
                      int64_t B, int64_t N, int64_t d, int64_t k, int kind, const float *logit_scale_dev,
                      void *stream);
/* The HEAD over a row window per query (leave-one-out prediction, one segment of a concatenated bank, "without
 * the query's own class" in a class-sorted bank): nw_fwd_f32's log-probabilities computed from the bank rows
 * that the query's window admits, and from no other.  row_lo / row_hi (B,) int32 on the device and exclude
 * mean what they mean for nw_knn_window_f32: row takes part when lo[b] <= row < hi[b] (exclude == 0), or when
 * it is outside that range (exclude != 0); lo >= hi is the empty window; the values are clamped to [0, N] on
 * the device and never used as an address.  The window is applied to the scores inside the tile kernel, before
 * the tile's maximum and exponentials: the result is the softmax over the admitted rows alone, not the full
 * softmax with terms subtracted (which cancels to nothing when an excluded row dominates).
 *   q         (B,d) fp32 queries
 *   s_split / s_scale / s_norm2   the bank as nw_split_rows_f16x2 leaves it ((N,d), (N,), (N,))
 *   sy        (N,) int64 labels; labels outside [0, C) are skipped as in nw_fwd_f32
 *   out       (B,C) fp32 log(p + 1e-12);  lse_out  optional (B,) fp32 log-sum-exp of the admitted scores
 * A query whose window admits no row: out[b, :] = log(1e-12) (every class absent), lse_out[b] = -inf, no NaN.
 * Always the split-fp16 tile kernel, at the tile height and with the raw-or-split-queries rule of
 * nw_knn_window_f32 at the same shape; no score matrix.  Regime: d % 32 == 0, 32 <= d <= 2^20, N > 25,
 * C >= 1, q, s_split and workspace 16-byte aligned; anything else returns NW_ERR_UNSUPPORTED before
 * anything is launched (callers mask a score matrix and call nw_aggregate_f32).  row_lo, row_hi, sy or out
 * NULL, or a negative size: NW_ERR_INVALID_ARG.  workspace: nw_fwd_workspace_bytes(B, N, d, C), else
 * NW_ERR_WORKSPACE.  B == 0: NW_OK.  No allocation, no synchronisation, no environment. */
int nw_fwd_window_f32(const float *q, const float *s_split, const float *s_scale, const float *s_norm2,
                      const int64_t *sy, const int32_t *row_lo, const int32_t *row_hi, int exclude,
                      float *out, float *lse_out, void *workspace, size_t workspace_bytes,
                      int64_t B, int64_t N, int64_t d, int64_t C, int kind, const float *logit_scale_dev,
                      void *stream);
/* Gradient of the head w.r.t. the QUERIES over a resident split bank, the bank a constant: no (B,N) buffer anywhere, no
 * support gradient.  The scores are recomputed tile by tile on the split-fp16 matrix cores (the forward's tile) and
 * contracted with the bank rows in the same kernel; the row window of nw_fwd_window_f32 is honoured, so the windowed head
 * (leave-one-out) is differentiable.
 *   q (B,d) fp32; s_split / s_scale / s_norm2: the bank of nw_split_rows_f16x2; sy (N,) int64;
 *   row_lo / row_hi (B,) int32: both NULL (no window) or both set, with `exclude` as in nw_fwd_window_f32;
 *   lse (B,), out (B,C): what the forward (nw_fwd_f32 with lse_out, or nw_fwd_window_f32) returned for these operands;
 *   gout (B,C): the upstream gradient;  gq (B,d): the result;  glogit_scale: optional scalar (0 unless clip).
 *   row_chunks: 0 lets the library choose how many chunks of support tiles share the bank; a positive value is
 *   clamped to the number of 64-row support tiles (the chunk reduction can then be exercised at small N).
 * A query whose window admits no row (lse = -inf) gets a zero row.  Two calls give identical bits (no float atomics).
 * Regime: nw_fwd_window_f32's -- d % 32 == 0, 32 <= d, N > 25, C >= 1, q / s_split / gq / workspace 16-byte aligned;
 * anything else is NW_ERR_UNSUPPORTED before anything is launched, and its workspace size is 0.  Null required pointers,
 * one of row_lo / row_hi alone, a negative size, clip without logit_scale_dev: NW_ERR_INVALID_ARG.  A short or NULL
 * workspace: NW_ERR_WORKSPACE.  B == 0: NW_OK.  No allocation, no synchronisation, no environment. */
size_t nw_bwd_query_workspace_bytes(int64_t B, int64_t N, int64_t d, int64_t C, int row_chunks);
int nw_bwd_query_f32(const float *q, const float *s_split, const float *s_scale, const float *s_norm2,
                     const int64_t *sy, const int32_t *row_lo, const int32_t *row_hi, int exclude,
                     const float *lse, const float *out, const float *gout,
                     float *gq, float *glogit_scale, void *workspace, size_t workspace_bytes,
                     int64_t B, int64_t N, int64_t d, int64_t C, int kind, const float *logit_scale_dev,
                     int row_chunks, void *stream);
/* SUPPORT WEIGHTS: the head with a prior weight w_j per bank row,
 *   out[b,c] = log( sum_{j admitted, sy_j = c} w_j exp(score_bj) / sum_{j admitted} w_j exp(score_bj) + 1e-12 ),
 * i.e. nw_fwd_window_f32 over the scores score_bj + a_j, a_j = log w_j: soft deletion and non-contiguous subsets of a live
 * bank (a_j = -inf removes row j from numerator and denominator alike), a flat class prior over an unbalanced bank
 * (a_j = -log n_class(j)), importance weights.  The weight is added in the tile epilogue, before the masks and the tile
 * maximum: no (B,N) matrix, and the maximum is that of the weighted scores.
 *   row_logw  (N,) fp32 on the device, required, 16-byte aligned: natural-log weights in the units of the scores.  Every
 *             value is finite or -inf.  NaN, +inf and magnitudes whose base-2 form (a * log2 e) overflows fp32 are outside
 *             the contract: the result for the queries that admit such a row is undefined, but nothing faults -- the value
 *             is never used as an address, and the library makes no device-side check and no synchronisation.
 *   row_lo / row_hi  both NULL (no window) or both set, with `exclude`, as in nw_fwd_window_f32 (exclude is ignored
 *             without a window).
 *   lse_out   optional (B,): log sum_{admitted} exp(score + a).
 * A DEAD query -- every admitted row has a = -inf, or the window is empty -- gets out = log(1e-12) in every class and
 * lse = -inf; no NaN anywhere.  With a = 0 everywhere the result is nw_fwd_window_f32's bit for bit.
 * Everything else -- operands, regime, alignment, tile height and raw-or-split-queries rule, workspace
 * (nw_fwd_workspace_bytes), status codes, refusals before anything is launched -- is nw_fwd_window_f32's; row_logw NULL
 * or one of row_lo / row_hi alone: NW_ERR_INVALID_ARG. */
int nw_fwd_weighted_f32(const float *q, const float *s_split, const float *s_scale, const float *s_norm2,
                        const int64_t *sy, const float *row_logw,
                        const int32_t *row_lo, const int32_t *row_hi, int exclude,
                        float *out, float *lse_out, void *workspace, size_t workspace_bytes,
                        int64_t B, int64_t N, int64_t d, int64_t C, int kind, const float *logit_scale_dev, void *stream);
/* nw_bwd_query_f32 for the weighted head: lse and out are nw_fwd_weighted_f32's for the same operands, weights and window.
 * The weights are a CONSTANT: there is no gradient with respect to row_logw.  They enter the softmax weight
 * W = exp(score + a - lse) only; the derivative of the score with respect to the query is taken at the raw score.  A dead
 * query (lse = -inf) gets a zero row of gq.  With a = 0 everywhere the result is nw_bwd_query_f32's bit for bit.
 * Regime, workspace (nw_bwd_query_workspace_bytes), row_chunks and status codes are nw_bwd_query_f32's; row_logw as above. */
int nw_bwd_query_weighted_f32(const float *q, const float *s_split, const float *s_scale, const float *s_norm2,
                              const int64_t *sy, const float *row_logw,
                              const int32_t *row_lo, const int32_t *row_hi, int exclude,
                              const float *lse, const float *out, const float *gout,
                              float *gq, float *glogit_scale, void *workspace, size_t workspace_bytes,
                              int64_t B, int64_t N, int64_t d, int64_t C, int kind, const float *logit_scale_dev,
                              int row_chunks, void *stream);
/* LEARNABLE support weights: nw_bwd_query_weighted_f32 with the gradient of the weighted head w.r.t. row_logw as well,
 *   glogw[j] = sum_b dS_bj,   dS_bj = W_bj (dP_b[sy_j] - t_b),   W_bj = exp(score_bj + a_j - lse_b)
 * -- the column sum over the queries of the quantity whose row contraction with the bank is gq, taken in the same kernel
 * from the same registers: no (B,N) buffer.  A row whose label is outside [0, C) has dP = 0 and gets -sum_b W_bj t_b.
 *   glogw  (N,) fp32, required, 16-byte aligned.  EVERY element of glogw[0..N) is written by every successful call with
 *          B > 0 (the caller never clears it); a row with a_j = -inf, a row that no query's window admits and the
 *          contribution of a dead query (lse = -inf) are exactly +0.0, no NaN.
 *   gq     (B,d) or NULL.  NULL is the weights-only variant (a frozen featurizer): the bank rows are not streamed a second
 *          time, no second product, and the workspace holds no partial gq tiles.  glogw of the two variants is the same
 *          bit for bit; with gq given, gq and glogit_scale are nw_bwd_query_weighted_f32's bits.
 *   glogit_scale  optional scalar in both variants (0 unless clip).
 * Reduction order: within a 64-query tile the 16 queries of a wave in a fixed exchange tree, then the four waves in
 * order; then the query tiles in ascending order (a finishing kernel).  Chunks own disjoint rows, so row_chunks does not
 * enter the sum: two calls, and calls with different row_chunks, give identical bits.  No float atomics.
 * workspace: nw_bwd_logw_workspace_bytes(B, N, d, C, row_chunks, want_gq) with want_gq = (gq != NULL); at most
 * ceil(B / 64) * 64 * ceil(N / 64) floats more than nw_bwd_query_workspace_bytes with gq, far fewer without.
 * Regime, alignment, row_chunks, status codes and refusals before anything is launched are nw_bwd_query_weighted_f32's;
 * glogw or row_logw NULL: NW_ERR_INVALID_ARG; a misaligned glogw: NW_ERR_UNSUPPORTED.  B == 0: NW_OK and NOTHING is
 * touched, glogw included (there is no query to sum over and no launch to write it: a caller with an empty batch clears
 * its own buffer). */
size_t nw_bwd_logw_workspace_bytes(int64_t B, int64_t N, int64_t d, int64_t C, int row_chunks, int want_gq);
int nw_bwd_query_logw_f32(const float *q, const float *s_split, const float *s_scale, const float *s_norm2,
                          const int64_t *sy, const float *row_logw,
                          const int32_t *row_lo, const int32_t *row_hi, int exclude,
                          const float *lse, const float *out, const float *gout,
                          float *gq, float *glogw, float *glogit_scale, void *workspace, size_t workspace_bytes,
                          int64_t B, int64_t N, int64_t d, int64_t C, int kind, const float *logit_scale_dev,
                          int row_chunks, void *stream);
/* VALUE HEAD: Nadaraya-Watson regression over a resident split bank, a real-valued target row per support instead of a label,
 *   out[b,t] = sum_{j admitted} exp(score_bj + a_j - lse_b) v_jt,
 * i.e. softmax(scores) @ values with no (B,N) buffer anywhere: regression targets, soft / smoothed / multi-hot labels, any
 * per-row attribute carried through the softmax.  The scores are recomputed tile by tile on the split-fp16 matrix cores and
 * contracted with the value rows in the same kernel (nw_bwd_query_f32's work split with the value rows in the bank's place).
 *   q (B,d) fp32; s_split / s_scale / s_norm2: the bank of nw_split_rows_f16x2;
 *   v_split / v_scale  (N,T), (N,): the VALUES as nw_split_rows_f16x2 leaves them (its norms output is not needed), T a
 *             multiple of 32 -- callers pad with zero columns.  Every value is FINITE, in every row, admitted or not: a row
 *             that takes no part has an exact 0 coefficient, and 0 x inf is NaN on the matrix pipe.  Nothing is checked on
 *             the device;
 *   row_logw  optional (N,) natural-log weights a_j, 16-byte aligned, under nw_fwd_weighted_f32's contract (finite or -inf);
 *             NULL: a = 0;
 *   row_lo / row_hi (B,) int32: both NULL (no window) or both set, with `exclude` as in nw_fwd_window_f32 (clamped to
 *             [0, N], never used as an address; exclude is ignored without a window);
 *   lse (B,): the log-sum-exp the forward returned for the SAME operands, weights and window (nw_fwd_window_f32 or
 *             nw_fwd_weighted_f32 with lse_out; a caller without labels passes all-zero labels and C = 1, one without a
 *             window the kept window [0, N)).  The weight is that forward's fused multiply-add, so the weights of a row sum
 *             to 1 to its tolerance;
 *   out (B,T) fp32: EVERY element is written by a successful call with B > 0;
 *   row_chunks: as in nw_bwd_query_f32 (0: the library chooses; a positive value is clamped to the 64-row tile count).
 * A dead query (lse = -inf) gets a zero row; a row at a = -inf, a row outside the window and the rows past N of the last tile
 * contribute exactly 0.  A finishing kernel adds the chunks' partial tiles in chunk order, scaled by exact powers of two: no
 * float atomics, two calls give identical bits.
 * Regime: nw_fwd_window_f32's for the operands -- d % 32 == 0, 32 <= d, N > 25 -- and T % 32 == 0, 32 <= T <= 16384; q,
 * s_split, v_split, out, row_logw and workspace 16-byte aligned; anything else is NW_ERR_UNSUPPORTED before anything is
 * launched, and the workspace size is then 0.  Null required pointers, one of row_lo / row_hi alone, a negative size or
 * row_chunks, clip without logit_scale_dev: NW_ERR_INVALID_ARG.  A short or NULL workspace
 * (nw_fwd_values_workspace_bytes(B, N, d, T, row_chunks)): NW_ERR_WORKSPACE.  B == 0: NW_OK.  No allocation, no
 * synchronisation, no environment. */
size_t nw_fwd_values_workspace_bytes(int64_t B, int64_t N, int64_t d, int64_t T, int row_chunks);
int nw_fwd_values_f32(const float *q, const float *s_split, const float *s_scale, const float *s_norm2,
                      const float *v_split, const float *v_scale, const float *row_logw,
                      const int32_t *row_lo, const int32_t *row_hi, int exclude,
                      const float *lse, float *out, void *workspace, size_t workspace_bytes,
                      int64_t B, int64_t N, int64_t d, int64_t T, int kind, const float *logit_scale_dev,
                      int row_chunks, void *stream);
/* The VALUE HEAD AT TRAINING TIME: the gradient of nw_fwd_values_f32 w.r.t. the QUERIES, the bank, the values and the
 * weights constants -- no (B,N) buffer anywhere, no gradient to the supports, the values or row_logw.  With g = gout,
 *   c_bj = g_b . v_j,   m_b = g_b . out_b,   dS_bj = W_bj (c_bj - m_b),   W_bj = exp(score_bj + a_j - lse_b),
 *   gq_b = sum_j dS_bj dscore_bj/dq_b          (the derivative taken at the raw score, as in nw_bwd_query_weighted_f32):
 * per 64-row support tile the scores are recomputed on the split-fp16 matrix cores, c is a second product of the same
 * kind over (gout, v_split, T), and dS is contracted with the bank rows in the same kernel (nw_bwd_query_f32's work split).
 *   q, s_split / s_scale / s_norm2, v_split / v_scale, row_logw, row_lo / row_hi / exclude: nw_fwd_values_f32's operands;
 *   lse (B,): the log-sum-exp that forward read;  out (B,T): the RAW output it wrote (not a logarithm of it);
 *   gout (B,T) fp32, 16-byte aligned: the upstream gradient w.r.t. out, zero in the padding columns of T;
 *   gq (B,d): the result, EVERY element written by a successful call with B > 0;  glogit_scale: optional scalar (0 unless clip);
 *   row_chunks: as in nw_bwd_query_f32.
 * A dead query (lse = -inf), a row outside the window, a row at a = -inf and the rows past N of the last tile contribute
 * exactly 0; an all-zero row of gout gives an all-zero row of gq; scaling a row of gout by a power of two scales its row of gq
 * exactly.  The value rows are finite in every row, as for the forward.  Chunks are added in chunk order by finishing kernels:
 * no float atomics, two calls give identical bits.
 * Accuracy: c - m cancels.  The error of c is ~2.4e-7 sum_t |g_t v_jt| whatever the spread of the values among the rows, so
 * value columns with a large common offset lose that many bits of the gradient: centre such columns.
 * Regime, alignment (gout and gq as well), status codes and refusals before anything is launched are nw_fwd_values_f32's;
 * out, gout or gq NULL: NW_ERR_INVALID_ARG.  workspace: nw_bwd_values_query_workspace_bytes(B, N, d, T, row_chunks), 0 for
 * a shape outside the regime; short or NULL: NW_ERR_WORKSPACE.  B == 0: NW_OK. */
size_t nw_bwd_values_query_workspace_bytes(int64_t B, int64_t N, int64_t d, int64_t T, int row_chunks);
int nw_bwd_values_query_f32(const float *q, const float *s_split, const float *s_scale, const float *s_norm2,
                            const float *v_split, const float *v_scale, const float *row_logw,
                            const int32_t *row_lo, const int32_t *row_hi, int exclude,
                            const float *lse, const float *out, const float *gout,
                            float *gq, float *glogit_scale, void *workspace, size_t workspace_bytes,
                            int64_t B, int64_t N, int64_t d, int64_t T, int kind, const float *logit_scale_dev,
                            int row_chunks, void *stream);
/* LEARNABLE VALUES AND SUPPORT WEIGHTS of the value head: the gradients of nw_fwd_values_f32 w.r.t. the VALUES and row_logw,
 *   gvalues[j,t] = sum_b W_bj g_bt,
 *   glogw[j]     = sum_b W_bj (g_b . v_j - m_b) = gvalues[j] . v_j - sum_b W_bj m_b,     m_b = g_b . out_b,
 * contractions over the QUERIES of the weights W_bj = exp(score_bj + a_j - lse_b) that nw_bwd_values_query_f32 recomputes:
 * a workgroup owns a 64-row support tile and a slab of value columns and loops over the 64-query tiles.  No (B,N) buffer,
 * no G V^T product, no float atomics.
 *   q, s_split / s_scale / s_norm2, row_logw, row_lo / row_hi / exclude, lse, out, gout: nw_bwd_values_query_f32's operands;
 *   v_rows   (N,T) the fp32 VALUES themselves (not split), 16-byte aligned, finite; read for glogw only, may be NULL without;
 *   gvalues  (N,T) fp32 or NULL, 16-byte aligned;  glogw (N,) fp32 or NULL, 16-byte aligned: at least one.  glogw requires
 *            row_logw and v_rows.  With gvalues == NULL (the weights-only mode) nothing of size N x T is stored or needed;
 *   query_chunks: 0 lets the library split the query loop when the support tiles alone cannot fill the chip; a positive
 *            value is clamped to the number of 64-query tiles.  Chunk partials are added in chunk order by a finish kernel.
 * EVERY element of gvalues[0..N) x [0..T) and of glogw[0..N) is written by a successful call with B > 0, nothing past them.
 * A row at a = -inf, a row no query's window admits and the share of a dead query (lse = -inf) are exactly +0.0 in every
 * column and in glogw; a zero column of gout gives a zero column of gvalues; the value rows do not enter gvalues.  Scaling
 * gout by a power of two scales gvalues exactly.  Two calls with the same arguments give the same bits.
 * Accuracy: W 2^15 and gout 2^E (E from max |gout|) are split into fp16 halves, products exact, sums fp32:
 *   |error of gvalues[j,t]| <~ (2^-21 + B 2^-24) sum_b W_bj |g_bt| + 2^-38 max|gout| sum_b W_bj.
 * Regime, alignment, status codes and refusals before anything is launched are nw_bwd_values_query_f32's; gvalues and glogw
 * both NULL, glogw without row_logw or v_rows: NW_ERR_INVALID_ARG.  workspace:
 * nw_bwd_values_support_workspace_bytes(B, N, d, T, query_chunks, want_gvalues) with want_gvalues = (gvalues != NULL), 0
 * for a shape outside the regime; short or NULL: NW_ERR_WORKSPACE.  B == 0: NW_OK and NOTHING is touched. */
size_t nw_bwd_values_support_workspace_bytes(int64_t B, int64_t N, int64_t d, int64_t T, int query_chunks, int want_gvalues);
int nw_bwd_values_support_f32(const float *q, const float *s_split, const float *s_scale, const float *s_norm2,
                              const float *v_rows, const float *row_logw,
                              const int32_t *row_lo, const int32_t *row_hi, int exclude,
                              const float *lse, const float *out, const float *gout,
                              float *gvalues, float *glogw, void *workspace, size_t workspace_bytes,
                              int64_t B, int64_t N, int64_t d, int64_t T, int kind, const float *logit_scale_dev,
                              int query_chunks, void *stream);
/* Gradient of the CLASS head over a resident split bank w.r.t. the BANK ROWS, without a (B,N) matrix (bwd_support.hip):
 *   gs_j = sum_b A_bj q_b + 2 (sum_b r_bj) s_j,  (A_bj, r_bj) the per-pair coefficients of nw_bwd_query_f32 (df/ddot and
 *   df/d|s|^2 times dS_bj = W_bj (dP_b[y_j] - t_b), the derivative taken at the RAW score, W carrying row_logw).
 *   q (B,d), s (N,d) the fp32 rows the split forms were prepared from (read for the 2 r s term only), s_split / s_scale /
 *   s_norm2 / sy / row_lo / row_hi / exclude / row_logw (or NULL) / lse / out / gout as nw_bwd_query_logw_f32;
 *   gs (N,d) fp32, 16-byte aligned;
 *   query_chunks: 0 lets the library split the query loop when the support tiles alone cannot fill the chip; a positive
 *            value is clamped to the number of 64-query tiles.  Chunk partials are added in chunk order by a finish kernel.
 * EVERY element of gs[0..N) x [0..d) is written by a successful call with B > 0, nothing past it.  A row at a = -inf, a row
 * no query's window admits and the share of a dead query (lse = -inf) are exactly 0.0 in every column.  Scaling gout by a
 * power of two scales gs exactly.  Two calls with the same arguments give the same bits.
 * Accuracy: A 2^E (E from the largest |A| a 64-row support tile has shown so far, accumulators rescaled exactly when it
 * rises) and q 2^F (F from max |q|) are split into fp16 halves, products exact, sums fp32; with Amax the tile's largest |A|:
 *   |error of gs[j,k]| <~ (2^-21 + B 2^-24) sum_b |A_bj| |q_bk| + 2^-38 (Amax sum_b |q_bk| + max|q| sum_b |A_bj|).
 * Regime, alignment, status codes and refusals before anything is launched are nw_bwd_query_f32's.  workspace:
 * nw_bwd_bank_support_workspace_bytes(B, N, d, C, query_chunks), 0 for a shape outside the regime; short or NULL:
 * NW_ERR_WORKSPACE.  B == 0: NW_OK and NOTHING is touched. */
size_t nw_bwd_bank_support_workspace_bytes(int64_t B, int64_t N, int64_t d, int64_t C, int query_chunks);
int nw_bwd_bank_support_f32(const float *q, const float *s, const float *s_split, const float *s_scale, const float *s_norm2,
                            const int64_t *sy, const float *row_logw,
                            const int32_t *row_lo, const int32_t *row_hi, int exclude,
                            const float *lse, const float *out, const float *gout,
                            float *gs, void *workspace, size_t workspace_bytes,
                            int64_t B, int64_t N, int64_t d, int64_t C, int kind, const float *logit_scale_dev,
                            int query_chunks, void *stream);
/* Gradient of the VALUE head over a resident split bank w.r.t. the BANK ROWS, without a (B,N) matrix (bwd_values_bank.hip):
 * learnable keys of a key-value memory (prototypes with regression targets, a condensed support set with soft labels).  With
 * g = gout and the values and the weights constants,
 *   c_bj = g_b . v_j,   m_b = g_b . out_b,   dS_bj = W_bj (c_bj - m_b),   W_bj = exp(score_bj + a_j - lse_b),
 *   gs_j = sum_b A_bj q_b + 2 (sum_b r_bj) s_j,  (A_bj, r_bj) the per-pair coefficients of nw_bwd_query_f32 (df/ddot and
 *   df/d|s|^2 times dS_bj, the derivative taken at the RAW score, W carrying row_logw):
 * nw_bwd_bank_support_f32 with c_bj - m_b in the place of dP_b[y_j] - t_b; c is a second product of the scores' kind over
 * (gout, v_split, T), recomputed per 64-query x 64-row tile as in nw_bwd_values_query_f32.
 *   q (B,d), s (N,d) the fp32 rows the split forms were prepared from (read for the 2 r s term only), s_split / s_scale /
 *   s_norm2, v_split / v_scale, row_logw (or NULL), row_lo / row_hi / exclude: nw_fwd_values_f32's operands;
 *   lse (B,), out (B,T): what that forward read and wrote for the same operands, window and weights (the RAW output);
 *   gout (B,T) fp32, 16-byte aligned: the upstream gradient w.r.t. out, zero in the padding columns of T;
 *   T: the padded width, a multiple of 32 within nw_bwd_values_support_f32's range;
 *   gs (N,d) fp32, 16-byte aligned;
 *   query_chunks: as in nw_bwd_bank_support_f32.
 * EVERY element of gs[0..N) x [0..d) is written by a successful call with B > 0, nothing past it; the padded columns of a
 * padded bank get zeros.  A row at a = -inf, a row no query's window admits and the share of a dead query (lse = -inf) are
 * exactly +0.0 in every column.  Every value must be finite, in every row: c of a pair that takes no part is multiplied with
 * W = 0.  Scaling gout by a power of two scales gs exactly.  No float atomics: two calls with the same arguments give the
 * same bits.
 * Accuracy: nw_bwd_bank_support_f32's bound for the contraction, with Amax the tile's largest |A|,
 *   |error of gs[j,k]| <~ (2^-21 + B 2^-24) sum_b |A_bj| |q_bk| + 2^-38 (Amax sum_b |q_bk| + max|q| sum_b |A_bj|),
 * on top of the error of dS: c - m cancels, and the error of c is ~2.4e-7 sum_t |g_t v_jt| whatever the spread of the values
 * among the rows, so value columns with a large common offset lose that many bits of the gradient: centre such columns.
 * Regime, alignment, order of the checks, status codes and refusals before anything is launched are
 * nw_bwd_values_support_f32's, for s and gs nw_bwd_bank_support_f32's.  workspace:
 * nw_bwd_values_bank_support_workspace_bytes(B, N, d, T, query_chunks) -- nothing of size B x N or N x T --, 0 for a shape
 * outside the regime; short or NULL: NW_ERR_WORKSPACE.  B == 0: NW_OK and NOTHING is touched. */
size_t nw_bwd_values_bank_support_workspace_bytes(int64_t B, int64_t N, int64_t d, int64_t T, int query_chunks);
int nw_bwd_values_bank_support_f32(const float *q, const float *s, const float *s_split, const float *s_scale,
                                   const float *s_norm2, const float *v_split, const float *v_scale, const float *row_logw,
                                   const int32_t *row_lo, const int32_t *row_hi, int exclude,
                                   const float *lse, const float *out, const float *gout,
                                   float *gs, void *workspace, size_t workspace_bytes,
                                   int64_t B, int64_t N, int64_t d, int64_t T, int kind, const float *logit_scale_dev,
                                   int query_chunks, void *stream);
/* support_influence (util/metric.py:23-50) of k SELECTED supports per query, from the head's own outputs:
 *   vals (B,k) fp32 raw scores and rows (B,k) int64 bank rows (a search's val_out / idx_out),
 *   sy (N,) int64, qy (B,) int64, out (B,C) log-probabilities and lse (B,) of nw_fwd_f32 over the same bank;
 *   infl_out (B,k) fp32, label_out optional (B,k) int64: the labels of the selected rows.
 * w = exp(val - lse[b]), p = exp(out[b, qy_b]), infl = log((p - p*w) / (p - w*[sy_row == qy_b])): the
 * arithmetic of nw_fwd_influence_f32's finishing pass, every product, difference and quotient rounded on
 * its own.  A slot whose row is outside [0, N) (the -1 of a padded search) gets influence +0.0, label -1.
 * One launch, no workspace.  Null pointers (label_out excepted) or a negative size: NW_ERR_INVALID_ARG;
 * k outside [1, 32]: NW_ERR_UNSUPPORTED; B == 0: NW_OK. */
int nw_influence_select_f32(const float *vals, const int64_t *rows, const int64_t *sy, const int64_t *qy,
                            const float *out, const float *lse, float *infl_out, int64_t *label_out,
                            int64_t B, int64_t k, int64_t N, int64_t C, void *stream);
/* Whether nw_fwd_f32 / nw_fwd_partial_f32 with split operands (s_split, d % 32 == 0) and no force_split
 * option run the split-fp16 tile kernel at this shape (1) or the fp32 one (0): the size rule alone.  For
 * callers that promise the bits of that call's scores_out, like nw_knn_f32's. */
int nw_scores_use_split(int64_t B, int64_t N, int64_t d);

/* ---------------------------------------------------------------------------------------------
 * The same search over a HALF-PRECISION bank (nw_pack_rows_f16): the neighbour modes of the reference
 * (KNN.__call__ / HNSW.__call__, nwhead/utils.py:185-216; NWNet.get_neighbors, nwhead/nw.py:245-249)
 * as an exact search over the fp16-rounded features, on the persistent 256-query tile kernel that
 * serves 'full' inference from such a bank.  Half the bank bytes and a third of the matrix work of
 * nw_knn_f32, no (B,N) score matrix, no second copy of the bank.
 *   q         (B,d) fp32 queries, already padded to the bank's width; rounded inside the call
 *   s_f16 / s_scale / s_norm2   the bank as nw_pack_rows_f16 leaves it ((N,d) fp16, (N,), (N,))
 *   idx_out   (B,k) int64 bank rows, best score first, equal fp32 scores in ascending row order
 *   val_out   optional (B,k) fp32: those very scores (the selection keys are made from the floats
 *             that are returned, so order and values cannot disagree)
 * The scores are those of the rounded query against the rounded rows, computed in fp32 from the packed
 * operands and the packed rows' norms.  They are not bit-equal to any other route's (the kernel rotates
 * its k chunks by the support tile, so equal rows in different tiles may differ in the last bits); they
 * do not depend on opts->persistent_wgs, and two calls give identical bits.
 * 1 <= k <= min(N, 32), d % 64 == 0, d >= 192, N > 25; anything else returns NW_ERR_UNSUPPORTED before
 * anything is launched, and nw_knn_f16_workspace_bytes returns 0 for it.  q, s_f16 and workspace
 * 16-byte aligned.  opts: NULL, or an nw_fwd_opts of which persistent_wgs is read.  B == 0: NW_OK.
 * ------------------------------------------------------------------------------------------- */
size_t nw_knn_f16_workspace_bytes(int64_t B, int64_t N, int64_t d, int64_t k);
int nw_knn_f16(const float *q, const void *s_f16, const float *s_scale, const float *s_norm2,
               int64_t *idx_out, float *val_out, void *workspace, size_t workspace_bytes,
               int64_t B, int64_t N, int64_t d, int64_t k, int kind, const float *logit_scale_dev,
               const nw_fwd_opts *opts, void *stream);

/* ---------------------------------------------------------------------------------------------
 * The k best supports per query over a bank SHARDED into G parts, each of which has been searched on
 * its own (nw_knn_f32 / nw_topk_f32), and the per-query k-nearest NW head over them: the cross-shard
 * step of the neighbour modes ('knn' / 'hnsw' with every query's own neighbours; NWNet.get_neighbors).
 * vals / rows / labels: (G, B, kc) each; shard g starts at base + g*stride_g (in 4-byte words).
 * Every (g, b) list is sorted best first. Equal scores are in ascending row order.
 * A slot with row < 0 is "no element" (a shard with fewer than kc rows, or an empty shard); it ends its list.
 * rows are GLOBAL bank rows (int32; rows are 31-bit), unique over the shards; labels are GLOBAL
 * class ids (int32).
 * Writes the k best per query: score descending (nw_topk_f32's order), equal scores by ascending global row.
 *   idx_out (B,k) int64, val_out (B,k) fp32 optional, label_out (B,k) int64 optional,
 *   out (B,C) fp32 optional:
 *     log( sum_{j<k, label_j == c} softmax_j(val[b, 0..k)) + 1e-12 )
 *     i.e. nw_aggregate_f32 of the merged (B,k) values with labels_batched = 1.
 *     A label outside [0,C) is treated exactly as that call treats it (its weight counts in the softmax's
 *     denominator and in no class).  Every element of out is written; a class without a neighbour gets log(1e-12).
 * 1 <= k <= 32, k <= kc <= 32, 1 <= G <= 64; anything else returns NW_ERR_UNSUPPORTED.
 * Null vals / rows / labels / idx_out, a negative size, or stride_g < B*kc with G > 1: NW_ERR_INVALID_ARG.
 * Fewer than k valid candidates for a query: the remaining slots get row -1, value -inf, label -1.
 * They take no part in the head.
 * One launch, one wave per query; no atomics: the result is bit-reproducible.  Like every entry: no
 * workspace, no allocation, no synchronisation, no environment.
 * ------------------------------------------------------------------------------------------- */
int nw_knn_merge_f32(const float *vals, const int32_t *rows, const int32_t *labels,
                     int64_t G, int64_t B, int64_t kc, int64_t stride_g, int64_t k, int64_t C,
                     int64_t *idx_out, float *val_out, int64_t *label_out, float *out, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Eval-mode BatchNorm (+ ReLU) of the pre-activation backbones as one pass: out = max(x * scale[c] +
 * shift[c], 0).  Replaces the BatchNorm2d -> ReLU pairs in front of the convolutions of
 * model/densenet.py:33-60 (_DenseLayer norm1/relu1), :82-91 (_Transition) and :139 + :160 (norm5 + relu)
 * at inference, where scale = gamma / sqrt(running_var + eps), shift = beta - running_mean * scale.
 *   x      n planes-of-c: element (i, ch, p) at x[i * x_batch_stride + ch * hw + p]  (the first c channels
 *          of a wider NCHW slab qualify: x_batch_stride >= c * hw)
 *   out    (n, c, hw) contiguous;  scale, shift (c,);  relu != 0 applies the max
 * ------------------------------------------------------------------------------------------- */
int nw_scale_shift_relu_f32(const float *x, const float *scale, const float *shift, float *out,
                            int64_t n, int64_t c, int64_t hw, int64_t x_batch_stride, int relu,
                            void *stream);
/* The same followed by a 2x2 / stride-2 average pool (floor sizes): out (n, c, h/2, w/2).  The transitions of the
 * DenseNets (norm - relu - conv 1x1 - avgpool, model/densenet.py:82-91, model/densenet3.py:25-35): the pool commutes
 * with the bias-free 1x1 convolution, so the folded inference copy pools first and convolves a quarter of the pixels. */
int nw_scale_shift_relu_avgpool2_f32(const float *x, const float *scale, const float *shift, float *out,
                                     int64_t n, int64_t c, int64_t h, int64_t w, int64_t x_batch_stride,
                                     int relu, void *stream);

/* out[r][c] = act(x[r][c] + bias[c] [+ residual[r][c]]) for a channels-last (NHWC) activation seen as (rows = n h w,
 * c): the folded BatchNorm bias, the identity of a ResNet block (model/resnet.py:58-66) and the ReLU behind a bias-free
 * convolution in one pass; c % 4 == 0, 16-byte aligned pointers, in place allowed (out == x). */
int nw_bias_act_nhwc_f32(const float *x, const float *bias, const float *residual, int relu, float *out,
                         int64_t rows, int64_t c, void *stream);

/* 1x1 convolution of the folded inference backbones with its neighbours fused in, on the fp32 matrix cores
 * (v_mfma_f32_16x16x4_f32: exact fp32 multiply-adds).  Replaces, in DenseNet's dense layers and transitions
 * (model/densenet.py:33-60 norm1-relu1-conv1-norm2-relu2, :82-91 norm-relu-conv) and CIFAR_DenseNet's
 * (model/densenet3.py:10-35), the scale-shift-ReLU pass, the GEMM, the bias add and the ReLU pass:
 *     out[n, co, p] = post( bias[co] + sum_ci W[co, ci] * pre(x[n, ci, p]) )
 *   x          (n, >= cin, hw) fp32, plane contiguous, batch stride x_batch_stride floats (a channel prefix of a
 *              dense-block slab is fine)
 *   pre_scale / pre_shift  optional (cin,): pre(v) = a_ci v + b_ci (eval-mode BatchNorm), then max(., 0) if pre_relu
 *   w_t        (cin rounded up to 16, cout) fp32: the weight TRANSPOSED, rows past cin ZERO (made once, when the
 *              inference copy is folded); cout % 4 == 0.  cout % 128 == 0 and hw % 4 == 0 select the LDS-DMA kernel
 *   workspace  nw_conv1x1_workspace_bytes(n, cin, cout, hw) bytes (partial tiles when K is split over workgroups:
 *              small planes); may be NULL when that is 0
 *   bias       optional (cout,) (the BatchNorm that FOLLOWS the convolution, folded); post_relu: max(., 0)
 *   out        (n, cout, hw), batch stride out_batch_stride floats */
size_t nw_conv1x1_workspace_bytes(int64_t n, int64_t cin, int64_t cout, int64_t hw);
int nw_conv1x1_f32(const float *x, int64_t x_batch_stride, const float *pre_scale, const float *pre_shift,
                   int pre_relu, const float *w_t, const float *bias, int post_relu, float *out,
                   int64_t out_batch_stride, void *workspace, size_t workspace_bytes,
                   int64_t n, int64_t cin, int64_t cout, int64_t hw, void *stream);

/* 3x3 convolution, stride 1, padding 1, as an implicit GEMM on the fp32 matrix cores with bias / residual / ReLU fused
 * in; the output may be a channel window of a wider tensor (out_batch_stride), e.g. a DenseNet block's slab.  Replaces
 * the 3x3 convolutions of the folded inference backbones (model/densenet.py:41-45 conv2, model/densenet3.py:10-22,
 * model/resnet.py:31-66 BasicBlock conv + folded BatchNorm + ReLU [+ identity]).
 *     out[n, co, y, x] = post( bias[co] + sum_{ci,ky,kx} W[co,ci,ky,kx] in[n, ci, y+ky-1, x+kx-1] [+ residual[n, co, y, x]] )
 *   x         (n, >= cin, H, W) fp32, planes contiguous, batch stride x_batch_stride floats
 *   w_t       (ceil(cin/8), 9, 8, cout) fp32: the weight re-laid out once at fold time,
 *             w_t[c / 8][3 ky + kx][c % 8][co] = W[co][c][ky][kx], channels past cin ZERO; cout % 32 == 0
 *   bias      optional (cout,); residual optional (n, cout, H, W) with its batch stride; post_relu: max(., 0) */
size_t nw_conv3x3_workspace_bytes(int64_t n, int64_t cin, int64_t cout, int64_t H, int64_t W);
int nw_conv3x3_f32(const float *x, int64_t x_batch_stride, const float *w_t, const float *bias,
                   const float *residual, int64_t res_batch_stride, int post_relu, float *out,
                   int64_t out_batch_stride, void *workspace, size_t workspace_bytes,
                   int64_t n, int64_t cin, int64_t cout, int64_t H, int64_t W, void *stream);
/* Workgroups nw_conv3x3_f32 launches for a shape (0: unsupported): 32-256 pixels x 32-128 output channels per
 * workgroup, 32 x 64 tiles with the K range shared by the workgroup's waves when the larger tiles would leave the
 * chip idle (small planes), their K range split over up to 8 workgroups when there are many input channels (7x7
 * planes: partial tiles in `workspace`, nw_conv3x3_workspace_bytes, added in order by a second kernel).  The folded
 * backbones keep MIOpen below 192. */
int64_t nw_conv3x3_workgroups(int64_t n, int64_t cin, int64_t cout, int64_t H, int64_t W);


/* ---------------------------------------------------------------------------------------------
 * Convolution of the backbones on the fp16 matrix cores at fp32-grade accuracy (csrc/conv_nhwc.hip): an implicit
 * GEMM over fp32 NHWC (torch channels_last) activations.  Replaces F.conv2d at model/resnet.py:31-66 (BasicBlock's
 * 3x3), :147-156 / :178-190 (strided 3x3 and the 1x1 projection of a stage's first block), model/densenet.py:33-60
 * (conv1 1x1, conv2 3x3), :82-91 (transition 1x1); a stride-1 convolution's data gradient (train.py:414) is the same
 * call on the flipped, transposed weight.
 *     y[n, yo, xo, co] = post( bias[co] + sum_{ky,kx,ci} W[co,ky,kx,ci] x[n, s yo + ky - pad, s xo + kx - pad, ci] [+ residual] )
 *   x         (n, H, W, Cin) fp32, Cin % 32 == 0 -- or few channels with KW * Cin <= 32 (the stems: Cin = 4 after
 *             nw_to_nhwc_pad_f32 is the fast form); the weight is then the (Cout, KH, 32) matrix [co][ky][kx * Cin + ci],
 *             zero-padded, through the same split
 *   amax_in   the amax record of x: NW_AMAX_SLOTS floats whose maximum is an upper bound on max|x| (nw_absmax_f32, or the
 *             amax_out of the call that wrote x; partial maxima per producing workgroup: no atomics, nothing to clear):
 *             the activations are split into fp16 pairs on the way into LDS with ONE power of two per tensor
 *   w_split, w_scale   the weight as (Cout, KH*KW*Cin) rows -- the bytes of a channels_last (Cout, Cin, KH, KW) tensor --
 *             through nw_split_rows_f16x2 (its third output, the row norms, is not used); Cout % 32 == 0
 *   bias      optional (Cout,);  residual optional (n, Ho, Wo, Cout);  relu != 0: max(., 0) (NaN kept)
 *   y         (n, Ho, Wo, Cout) fp32;  amax_out optional: the amax record of y (NW_AMAX_SLOTS floats, all written)
 *   ldx, ldy  floats between consecutive pixels of x / y (0: Cin / Cout, dense): a channel window of a wider NHWC tensor
 *             as input or output (a dense block's slab, model/densenet.py:62-80, takes each layer's 32 channels in place);
 *             residual stays dense
 * nw_conv2d_nhwc_supported: 1 when the shape is served (else nw_conv2d_nhwc_f16x2 returns NW_ERR_UNSUPPORTED).
 * ------------------------------------------------------------------------------------------- */
#define NW_AMAX_SLOTS 256
int nw_absmax_f32(const float *x, int64_t count, float *amax_out, void *stream);
/* x (n, c, hw) fp32 with element strides (stride_n, stride_c, stride_p) -- NCHW or channels_last -- to y (n, hw, cp)
 * channels-last with the channels c .. cp-1 zero (cp % 4 == 0), and amax_out <- max|x|: the network input as the
 * 4-channel NHWC tensor the 7x7 stems (model/resnet.py:147, model/densenet.py:118) read pixel by aligned pixel. */
int nw_to_nhwc_pad_f32(const float *x, float *y, float *amax_out, int64_t n, int64_t c, int64_t hw, int64_t cp,
                       int64_t stride_n, int64_t stride_c, int64_t stride_p, void *stream);
int nw_conv2d_nhwc_supported(int64_t n, int64_t H, int64_t W, int64_t Cin, int64_t Cout, int64_t KH, int64_t KW,
                             int64_t stride, int64_t pad);
int nw_conv2d_nhwc_f16x2(const float *x, const float *amax_in, const float *w_split, const float *w_scale,
                         const float *bias, const float *residual, int relu, float *y, float *amax_out,
                         int64_t n, int64_t H, int64_t W, int64_t Cin, int64_t Cout, int64_t KH, int64_t KW,
                         int64_t stride, int64_t pad, int64_t ldx, int64_t ldy, float *moments, void *stream);
/* moments (nullable, Cin % 32 == 0): the convolution also leaves BatchNorm's batch statistics of y, so the BatchNorm that
 * follows (model/densenet.py:33-60: conv1 -> norm2; the next layers' norm1 over conv2's channels) needs no pass over y:
 * per group g of output pixels and channel co, moments[(k G + g) Cout + co] = k 0: pixels in the group, 1: their mean,
 * 2: the sum of squared deviations from it, 3: their minimum, 4: their maximum; G = nw_conv2d_nhwc_moments_groups(same shape
 * arguments) groups (5 G Cout floats), merged by nw_bn_nhwc_moments_from_partials_f32 / nw_bn_nhwc_prep_from_partials_f32. */
/* Round 4 -- BatchNorm + ReLU in front of a convolution, applied by the convolution's loaders on the way into LDS
 * (model/densenet.py:36-45: norm1 -> relu1 -> conv1, norm2 -> relu2 -> conv2 without the tensors in between;
 * :86-90 likewise): y = conv(relu((x - mean) a + beta)), a = gamma / sqrt(var + eps).
 *   pre      3 Cin floats: mean | a | beta of the Cin channels the convolution reads (nw_bn_nhwc_prep_f32 /
 *            nw_bn_nhwc_prep_from_partials_f32 make it; an inference caller fills it from the running statistics)
 *   amax_in  raw_records == 0: ONE amax record bounding |relu((x - mean) a + beta)| (the same two entries leave the exact
 *            bound; any upper bound is legal).  raw_records = n > 0 (an inference caller without batch statistics): n
 *            consecutive amax records of the RAW tensor x -- those of its producers: a dense block's input and every layer's
 *            output so far -- and the kernel derives the bound itself, max_c |a_c| (A + |mean_c|) + max(beta_c, 0) with A the
 *            records' maximum
 *   bias / relu: the inference epilogue (a folded BatchNorm behind the convolution); moments: as nw_conv2d_nhwc_f16x2.
 * `moments` of this and of nw_conv2d_nhwc_f16x2 hold FIVE rows per group since round 4: count, mean, M2, minimum,
 * maximum (5 G Cout floats). */
int nw_conv2d_nhwc_bnrelu_f16x2(const float *x, const float *pre, const float *amax_in, int64_t raw_records,
                                const float *w_split, const float *w_scale, const float *bias, int relu, float *y,
                                float *amax_out, int64_t n,
                                int64_t H, int64_t W, int64_t Cin, int64_t Cout, int64_t KH, int64_t KW, int64_t stride,
                                int64_t pad, int64_t ldx, int64_t ldy, float *moments, void *stream);
int64_t nw_conv2d_nhwc_moments_groups(int64_t n, int64_t H, int64_t W, int64_t Cin, int64_t Cout, int64_t KH, int64_t KW,
                                      int64_t stride, int64_t pad);

/* ---------------------------------------------------------------------------------------------
 * Training-mode BatchNorm2d (+ ReLU) in front of / behind the backbones' convolutions, forward and
 * backward, one kernel each (torch: batch-norm kernels + a relu kernel each way).  Same call sites as
 * nw_scale_shift_relu_f32 plus the conv -> bn -> relu pairs of model/resnet.py:31-66; the backward is what
 * autograd derives for relu(batch_norm(x)) at train.py:414.
 *   forward : batch statistics per channel over (n, hw); y = max(gamma (x - mean) / sqrt(var + eps) + beta, 0);
 *             running_mean/var (nullable) updated in place with `momentum` (unbiased variance), the int64
 *             num_batches_tracked counter (nullable) incremented, save_mean / save_invstd (c,) written for the
 *             backward
 *   backward: dx (n, c, hw), dgamma (c,), dbeta (c,) from dy (n, c, hw) contiguous; the ReLU mask is recomputed
 *             from x, nothing else is saved
 *   residual (nullable, (n, c, hw) contiguous): y = max(bn(x) + residual, 0), the tail of a ResNet block
 *             (model/resnet.py:58-66, :100-108); the backward then also writes dresidual (the masked dy)
 *   acc (nullable, backward): a second gradient of x, element (i, ch, p) at acc[i * acc_batch_stride + ch * hw + p],
 *             added into dx (the running concatenation of a dense block, model/densenet.py:62-80, feeds this
 *             BatchNorm and the next concatenation: autograd would add the two with a strided kernel of its own)
 *   x element (i, ch, p) at x[i * x_batch_stride + ch * hw + p]; y, dy, dx contiguous
 * ------------------------------------------------------------------------------------------- */
int nw_bn_relu_train_fwd_f32(const float *x, const float *residual, const float *gamma, const float *beta, float *running_mean,
                             float *running_var, float *y, float *save_mean, float *save_invstd,
                             int64_t *num_batches_tracked, int64_t n, int64_t c, int64_t hw,
                             int64_t x_batch_stride, float momentum, float eps, int relu, void *stream);
int nw_bn_relu_train_bwd_f32(const float *x, const float *residual, const float *dy, const float *gamma,
                             const float *beta, const float *save_mean, const float *save_invstd, float *dx,
                             float *dresidual, float *dgamma, float *dbeta, const float *acc,
                             int64_t acc_batch_stride, int64_t n, int64_t c, int64_t hw,
                             int64_t x_batch_stride, int relu, void *stream);

/* Every convolution weight of a network to the split-row operands nw_conv2d_nhwc_f16x2 reads, in ONE launch (the weights
 * change with every optimizer step, train.py:414-415).  jobs: device array of njobs x 10 int64 --
 *   [0] address of a torch-contiguous (Cout, Cin, KH, KW) fp32 weight, [1] offset (floats) of the operand in split_base,
 *   [2] offset of its row scales in scale_base, [3] index of its first row among all rows (ascending), [4] rows, [5] cols
 *   (floats per row, % 32 == 0), [6] Cin, [7] Cout, [8] KH * KW, [9] KW | mode << 32 with
 *   mode 0: the forward operand, rows = Cout, row co = [tap][ci];  mode 1: the data-gradient operand of a stride-1
 *   convolution, rows = Cin, row ci = [flipped tap][co];  mode 2: few input channels (Cin <= 4), rows = Cout,
 *   row co = [ky][32 floats: kx * 4 + ci, zero-padded] (the operand of the stems over a 4-channel input). */
int nw_split_conv_weights_f16x2(const int64_t *jobs, int64_t njobs, int64_t total_rows, float *split_base,
                                float *scale_base, void *stream);

/* Weight gradient of a stride-1 'same' convolution (1x1, or 3x3 with padding 1) over channels-last activations on the fp16
 * matrix cores (csrc/conv_wgrad.hip): what autograd derives for the weight of F.conv2d at model/densenet.py:33-60, :82-91
 * and model/resnet.py:31-66 in loss.backward() (train.py:414).
 *     dw[co, ky, kx, ci] = sum_{n,y,x} gy[n, y, x, co] * x[n, y + ky - pad, x + kx - pad, ci]
 *   x (n, H, W, Cin), gy (n, H, W, Cout) fp32 with their amax records; Cin % 8 == 0, Cout % 8 == 0; ldx, ldg: floats
 *   between consecutive pixels of x / gy (0: dense)
 *   dw (Cout, KH, KW, Cin) fp32: the bytes of a channels_last (Cout, Cin, KH, KW) tensor
 *   workspace: nw_conv2d_nhwc_wgrad_workspace_bytes(...) (partial tiles of the position chunks, added in order)
 * nw_conv2d_nhwc_wgrad_supported: 1 when the shape is served, else the call returns NW_ERR_UNSUPPORTED. */
int nw_conv2d_nhwc_wgrad_supported(int64_t n, int64_t H, int64_t W, int64_t Cin, int64_t Cout, int64_t KH, int64_t KW,
                                   int64_t stride, int64_t pad);
size_t nw_conv2d_nhwc_wgrad_workspace_bytes(int64_t n, int64_t H, int64_t W, int64_t Cin, int64_t Cout, int64_t KH,
                                            int64_t KW, int64_t stride, int64_t pad);
int nw_conv2d_nhwc_wgrad_f16x2(const float *x, const float *amax_x, const float *gy, const float *amax_g, float *dw,
                               void *workspace, size_t workspace_bytes, int64_t n, int64_t H, int64_t W, int64_t Cin,
                               int64_t Cout, int64_t KH, int64_t KW, int64_t stride, int64_t pad, int64_t ldx, int64_t ldg,
                               void *stream);
/* Several independent weight gradients in as few launches as possible (all 3x3 problems in one kernel, all 1x1 problems in
 * another, 32 per launch): the layers of a dense block on 14x14 / 7x7 maps give a dozen workgroups each, and their weight
 * gradients are not on the backward's critical path -- collected per block and run together they fill the chip.  Each job
 * as in nw_conv2d_nhwc_wgrad_f16x2; workspace: nw_conv2d_nhwc_wgrad_batch_workspace_bytes(jobs, njobs) (every job its own
 * part).  Nothing is launched if any job is refused. */
typedef struct nw_wgrad_job {
    const float *x, *amax_x, *gy, *amax_g;
    float *dw;
    int64_t n, H, W, Cin, Cout, KH, KW, stride, pad, ldx, ldg;
    int64_t out_oihw;   /* != 0: dw in torch's contiguous (Cout, Cin, KH, KW) layout instead of (Cout, KH, KW, Cin) */
    const float *pre_x; /* nullable: 3 Cin floats mean | a | beta -- the x operand is relu((x - mean) a + beta), as the forward
                           convolution read it (nw_conv2d_nhwc_bnrelu_f16x2); amax_x then bounds THAT tensor */
    /* rowrun_stride = s > 0 (round 4: the strided few-channel stems, model/densenet.py:114-116, model/resnet.py:147): the weight
     * gradient of a KH x KW convolution over a 4-channel NHWC input x (in_H x in_W pixels; RGB zero-padded to four channels) as
     * ONE 1x1 problem over gy's grid (H, W = output size, KH = KW = 1, stride 1, pad 0) with Cin = 32 KH "channels": channel
     * 32 ky + 4 kx + ci of output pixel (yo, xo) is x[s yo + row0 + ky][s xo + col0 + kx][ci] (zero outside the image; row0 =
     * col0 = -padding).  dw (Cout, 32 KH): [co][32 ky + 4 kx + ci]; the columns with kx >= KW or ci = 3 are not part of dW. */
    int64_t rowrun_stride, in_H, in_W, row0, col0;
} nw_wgrad_job;
size_t nw_conv2d_nhwc_wgrad_batch_workspace_bytes(const nw_wgrad_job *jobs, int64_t njobs);
int nw_conv2d_nhwc_wgrad_batch_f16x2(const nw_wgrad_job *jobs, int64_t njobs, void *workspace, size_t workspace_bytes,
                                     void *stream);
/* device address of 32 bytes of zeros the convolution kernels read in place of pixels that do not exist (internal) */
const void *nw_conv_zero_page(void);

/* ---------------------------------------------------------------------------------------------
 * The same pair over channels-last activations (csrc/bn_nhwc.hip), for the training path whose convolutions run in
 * nw_conv2d_nhwc_f16x2: x is (rows = n h w, c) with row stride ldx >= c floats (a channel prefix of a wider NHWC
 * tensor qualifies), c % 4 == 0 and c <= 2560 (NW_ERR_UNSUPPORTED beyond: the per-channel factors live in LDS), y / dy / dx
 * dense (rows, c).  Moments per row chunk merged in a fixed order (Chan),
 * deterministic; amax_out (nullable): the amax record (NW_AMAX_SLOTS floats) of y / dx for the convolution that reads
 * it next.  acc (nullable, backward): a second gradient of x with row stride ldacc, added into dx; lddx: row stride of
 * dx (0: dense); dx may be acc itself (the gradient slab of a dense block accumulates in place).
 * workspace: nw_bn_nhwc_workspace_bytes(rows, c).
 * ------------------------------------------------------------------------------------------- */
size_t nw_bn_nhwc_workspace_bytes(int64_t rows, int64_t c);
int nw_bn_relu_nhwc_train_fwd_f32(const float *x, int64_t ldx, const float *gamma, const float *beta, float *running_mean,
                                  float *running_var, float *y, float *save_mean, float *save_invstd,
                                  int64_t *num_batches_tracked, float *amax_out, void *workspace, size_t workspace_bytes,
                                  int64_t rows, int64_t c, float momentum, float eps, int relu, void *stream);
/* The forward in phases, for a caller that has the batch statistics from elsewhere (a dense block: a channel's statistics
 * are the same for every later layer's norm1, and a convolution's epilogue leaves the moments of what it writes):
 *   nw_bn_nhwc_moments_f32                mean, 1/sqrt(var + eps), biased var of the c channels of x (c,) each
 *   nw_bn_nhwc_moments_from_partials_f32  the same from the groups a convolution left (nw_conv2d_nhwc_f16x2's `moments`)
 *   nw_bn_relu_nhwc_apply_f32             y = act((x - mean) gamma invstd + beta) + the amax record of y; updates THIS
 *                                         layer's running statistics (momentum; unbiased var) and step counter */
int nw_bn_nhwc_moments_f32(const float *x, int64_t ldx, int64_t rows, int64_t c, float eps, float *mean, float *invstd,
                           float *var, void *workspace, size_t workspace_bytes, void *stream);
int nw_bn_nhwc_moments_from_partials_f32(float *partials, int64_t groups, int64_t c, float eps, float *mean,
                                         float *invstd, float *var, void *stream);
/* Round 4: what a convolution that applies the BatchNorm itself needs (nw_conv2d_nhwc_bnrelu_f16x2).
 *   nw_bn_nhwc_moments_minmax_f32        nw_bn_nhwc_moments_f32 + every channel's minimum and maximum
 *                                        (workspace: nw_bn_nhwc_minmax_workspace_bytes)
 *   nw_bn_nhwc_prep_from_partials_f32    statistics (mean, invstd, var, vmin, vmax) from a convolution's 5-row `moments`
 *                                        and, with gamma != NULL, the table `tab` (3 c floats mean | a | beta), the exact
 *                                        bound on |act((x - mean) a + beta)| as an amax record, the layer's running
 *                                        statistics (nullable) and step counter (nullable), in the same launch
 *   nw_bn_nhwc_prep_f32                  the table and bound from statistics that exist (rows = samples per channel) */
int nw_bn_nhwc_moments_minmax_f32(const float *x, int64_t ldx, int64_t rows, int64_t c, float eps, float *mean, float *invstd,
                                  float *var, float *vmin, float *vmax, void *workspace, size_t workspace_bytes, void *stream);
size_t nw_bn_nhwc_minmax_workspace_bytes(int64_t rows, int64_t c);
int nw_bn_nhwc_prep_from_partials_f32(float *partials, int64_t groups, int64_t c, float eps, float *mean, float *invstd,
                                      float *var, float *vmin, float *vmax, const float *gamma, const float *beta,
                                      float *running_mean, float *running_var, int64_t *num_batches_tracked, float momentum,
                                      int relu, float *tab, float *amax_out, void *stream);
/* ... the same where the fresh channels are a WINDOW [offset, offset + c) of wider statistics arrays (a dense block's slab:
 * mean .. vmax are the slab-wide arrays) and the BatchNorm to prepare (gamma, beta, running statistics: offset + c channels) also
 * reads the n_old <= offset channels in front of it, whose statistics exist: one launch does both (rows: samples per channel). */
int nw_bn_nhwc_prep_window_from_partials_f32(float *partials, int64_t groups, int64_t c, int64_t offset, int64_t n_old, int64_t rows,
                                             float eps, float *mean, float *invstd, float *var, float *vmin, float *vmax,
                                             const float *gamma, const float *beta, float *running_mean, float *running_var,
                                             int64_t *num_batches_tracked, float momentum, int relu, float *tab, float *amax_out,
                                             void *stream);
int nw_bn_nhwc_prep_f32(const float *mean, const float *invstd, const float *var, const float *vmin, const float *vmax,
                        const float *gamma, const float *beta, float *running_mean, float *running_var,
                        int64_t *num_batches_tracked, float momentum, int relu, int64_t rows, int64_t c, float *tab,
                        float *amax_out, void *stream);
int nw_bn_relu_nhwc_apply_f32(const float *x, int64_t ldx, const float *mean, const float *invstd, const float *var,
                              const float *gamma, const float *beta, float *running_mean, float *running_var,
                              int64_t *num_batches_tracked, float momentum, float *y, float *amax_out, int64_t rows,
                              int64_t c, int relu, void *stream);
/* The ImageNet stems at inference in one kernel (csrc/stem_pool.hip; model/resnet.py:147, :200-203, model/densenet.py:114-120 with
 * the BatchNorm folded into weight and bias): y = maxpool3x3/2/1(relu(conv7x7/2/3(x) + bias)), 64 output channels; the
 * 112 x 112 map between the two never reaches memory.
 *   x4 (n, H, W, 4) fp32: the 4-channel padded input of nw_to_nhwc_pad_f32, amax_in its amax record;
 *   w_split / w_scale: the (64, 7 x 32) few-channel operand of nw_split_rows_f16x2 (k = 32 ky + 4 kx + ci, as nw_conv2d_nhwc_f16x2
 *     takes it for a 4-channel input); bias (64,);
 *   y (n, Hp, Wp, >= 64) with row stride ldy floats (0: 64), Hp = ((H - 1) / 2 + 1 - 1) / 2 + 1; amax_out (nullable): its record.
 * Same values as nw_conv2d_nhwc_f16x2(bias, relu) + nw_maxpool3x3s2_nhwc_f32 up to fp32 summation order. */
int nw_stem7x7s2_relu_maxpool_supported(int64_t n, int64_t H, int64_t W, int64_t cout);
int nw_stem7x7s2_relu_maxpool_f16x2(const float *x4, const float *amax_in, const float *w_split, const float *w_scale,
                                    const float *bias, float *y, float *amax_out, int64_t n, int64_t H, int64_t W, int64_t ldy,
                                    void *stream);
/* An eval-mode DenseNet transition's BatchNorm + ReLU with its 2 x 2 average pool in front of the bias-free 1 x 1 convolution
 * (model/densenet.py:83-91 runs norm -> relu -> conv -> pool; pool and convolution commute): y = avgpool2x2(relu((x - mean) a + beta)),
 * tab = mean | a | beta (c floats apart), rows of x / y may be strided (ldx, ldy; 0: c); amax_out (nullable): the record of y. */
int nw_bn_relu_avgpool2x2_nhwc_f32(const float *x, int64_t ldx, const float *tab, float *y, int64_t ldy, float *amax_out,
                                   int64_t n, int64_t h, int64_t w, int64_t c, void *stream);
/* The end of a residual block in training (model/resnet.py:60-66, :100-108: out = relu(bn(.) + identity)) over two tensors of
 * equal layout, `count` floats each (a multiple of 4), 16-byte aligned: nw_add_relu_f32 writes out = relu(a + b) (x < 0 ? 0 : x:
 * keeps a NaN) and out's amax record; nw_relu_bwd_f32 writes dx = g where out > 0, else 0 -- the gradient of BOTH summands --
 * and dx's amax record.  amax_out nullable. */
int nw_add_relu_f32(const float *a, const float *b, float *out, float *amax_out, int64_t count, void *stream);
int nw_relu_bwd_f32(const float *out, const float *g, float *dx, float *amax_out, int64_t count, void *stream);
int nw_bn_relu_nhwc_train_bwd_f32(const float *x, int64_t ldx, const float *dy, const float *gamma, const float *beta,
                                  const float *save_mean, const float *save_invstd, float *dx, float *dgamma,
                                  float *dbeta, const float *acc, int64_t ldacc, int64_t lddx, float *amax_out,
                                  void *workspace, size_t workspace_bytes, int64_t rows, int64_t c, int relu, void *stream);

/* ---------------------------------------------------------------------------------------------
 * The pools of the backbones' training path over channels-last fp32 activations (csrc/pool_nhwc.hip): the 2 x 2 / 2
 * average pool of a DenseNet transition (reference model/densenet.py:83-91, nn.AvgPool2d(2, 2): an odd last row / column
 * is dropped) and the 3 x 3 / 2 pad 1 max pool of the stems (model/densenet.py:114, model/resnet.py:147; torch's scan:
 * a later value of the window wins when it is greater or NaN).  x (n, h, w, c), c % 4 == 0, rows may be strided (ld* >= c
 * floats, 0: dense): a pool can read from / write into a channel prefix of a wider NHWC tensor.  The max pool leaves the
 * winning tap (ky * 3 + kx) of every output value in `tap` ((n, ho, wo, c) bytes, dense; nullable: inference), which is all its backward needs
 * beside gy; both backwards are gathers over the input pixels (no atomics, deterministic) and write every value of gx.
 * ------------------------------------------------------------------------------------------- */
int nw_avgpool2x2_nhwc_f32(const float *x, int64_t ldx, float *y, int64_t ldy, int64_t n, int64_t h, int64_t w, int64_t c,
                           void *stream);
int nw_avgpool2x2_nhwc_bwd_f32(const float *gy, int64_t ldgy, float *gx, int64_t ldgx, int64_t n, int64_t h, int64_t w,
                               int64_t c, void *stream);
int nw_maxpool3x3s2_nhwc_f32(const float *x, int64_t ldx, float *y, int64_t ldy, unsigned char *tap, int64_t n, int64_t h,
                             int64_t w, int64_t c, void *stream);
int nw_maxpool3x3s2_nhwc_bwd_f32(const float *gy, int64_t ldgy, const unsigned char *tap, float *gx, int64_t ldgx, int64_t n,
                                 int64_t h, int64_t w, int64_t c, void *stream);

/* ---------------------------------------------------------------------------------------------
 * The optimizer step of the training harness (reference train.py:243-247: torch.optim.SGD(momentum 0.9, weight decay,
 * nesterov)) for all parameter tensors of a network in a few launches (csrc/sgd.hip; 96 tensors per launch, their addresses
 * in the kernel arguments).  Per element, torch's formula with dampening 0:
 *   g = grad + weight_decay p;  buf = init_buf ? g : momentum buf + g;  p -= lr (nesterov ? g + momentum buf : buf)
 * momentum == 0: no buffer is read or written (momentum_buf may be NULL).  init_buf != 0: the first step of these
 * parameters (torch clones the gradient into the buffer).  fp32, any length; tensors 16-byte aligned take the vector path.
 * ------------------------------------------------------------------------------------------- */
typedef struct nw_sgd_param {
    float *param;
    const float *grad;
    float *momentum_buf;
    int64_t n;
} nw_sgd_param;
int nw_sgd_step_f32(const nw_sgd_param *params, int64_t nparams, float lr, float momentum, float weight_decay, int nesterov,
                    int init_buf, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Diagnostics (no reference counterpart): device time of the TILE kernel alone -- the kernel the
 * roofline is quoted on (nw_fused_kernel / nw_fused_f16p_kernel), without the small kernels around
 * it (query split, run tables, merge).  While enabled, every forward brackets its tile-kernel launch
 * with two HIP events on the launch stream; nw_debug_tile_timing_read waits for them, returns their
 * summed elapsed time and the number of launches since the last read, and clears both.
 * ------------------------------------------------------------------------------------------- */
int nw_debug_tile_timing(int enable);
/* Diagnostic knobs (timing experiments; process-wide; never needed in normal use).  Names: pvar, qg, tile_rs,
 * no_persistent, split_queries, bwd_no_mfma, bwd_split, xgemm_wgs, split_lbits, conv_max_wgs, conv_skip_cfgs,
 * conv_force_cfg; any other name is refused with NW_ERR_INVALID_ARG.  The Python layer forwards the
 * NW_<NAME> environment variables once, when it loads the library; the library itself never reads the environment. */
int nw_debug_set(const char *name, int value);
int nw_debug_tile_timing_read(double *total_us, int64_t *launches);
/* The launch decision of the fused head for one call, as the library would take it (plan_fused, csrc/fused.hip): no launch,
 * no device needed.  form: 0 fp32 supports, 1 split rows, 2 half-precision rows.  outputs: 0 log-probabilities or partials,
 * 1 the same plus scores, 2 the k best candidates per query (nw_knn_f32).  norms: support norms supplied.  cus: CU count to
 * plan for, 0 = the current device's (256 when there is none), at most 2^20.  Returns NW_OK when *plan was filled; plan->status is what
 * the launch itself would return for the combination.  mode: 0 register-staged fp32, 1 LDS-DMA fp32, 2 LDS-DMA fp32 with
 * the caller's norms, 3 split operands, 4 split supports and raw queries; out: as `outputs`.  variant / workgroups / qgroup
 * describe the persistent kernel and are 0 without it. */
typedef struct nw_fwd_plan {
    int32_t status;
    int32_t rs, bs, n_stiles, n_qtiles, grid;   /* tile height in 16-row blocks and in rows; support / 64-query tiles; workgroups */
    int32_t mode, out;
    int32_t dma, persistent, variant, workgroups, qgroup;
    int32_t split_queries, run_tables;          /* a query split / pack launch, run tables before the tile kernel */
    int32_t reserved;
    uint64_t lds_bytes;                         /* dynamic LDS of the tile kernel */
} nw_fwd_plan;
int nw_debug_fwd_plan(int64_t B, int64_t N, int64_t d, int64_t C, int form, int outputs, int k, int norms, int kind,
                      int persistent_wgs, int cus, nw_fwd_plan *plan);
/* The map of the forward workspace (nw_fwd_workspace_bytes) for one shape, as every forward entry point carves it: no launch,
 * no device needed.  Six areas in this order, each starting on a multiple of 256 bytes where the one before ends, the last
 * ending at `total`: 0 main (the (B,N) scores or the fused partials), 1-3 rows, scales and norms of the split / packed
 * queries, 4 the log-sum-exp slot, 5 the slice partials of the sliced aggregation (empty when n_slices == 1).
 * NW_ERR_INVALID_ARG for a null pointer or a negative size; B <= 0 or N <= 0: all zeros. */
#define NW_FWD_AREAS 6
typedef struct nw_fwd_layout {
    uint64_t off[NW_FWD_AREAS], bytes[NW_FWD_AREAS];
    uint64_t total;                             /* == nw_fwd_workspace_bytes(B, N, d, C) */
    int32_t n_slices, reserved;
} nw_fwd_layout;
int nw_debug_fwd_layout(int64_t B, int64_t N, int64_t d, int64_t C, nw_fwd_layout *layout);
/* The plan of the head's backward (nw_bwd_f32 / nw_bwd_bank_f32) for one shape, as the launcher takes it under the current
 * knobs: no launch, no device needed.  status: what the launcher would answer once its arguments and workspace are in order
 * (NW_ERR_UNSUPPORTED when the coefficient kernel's LDS exceeds 160 KiB).  route: 0 VALU, 1 fp32 matrix cores, 2 split
 * fp16 (== nw_bwd_uses_split).  ld: row stride of the coefficient matrices; Bpad: rows of the split queries.  gq_* / gs_*:
 * K-split of the two products (0 on the VALU route).  Fifteen areas of the workspace in this order, each starting on a
 * multiple of 256 bytes where the one before ends, the last ending at `total`, an area the route does not use empty:
 * 0 A, 1 Rs, 2 rq, 3 gls, 4 qn2, 5 sn2, 6 rs, 7 s_split, 8 s_scale, 9 q_split, 10 ascale, 11 qv, 12 gfac, 13 part (partial
 * tiles of gq), 14 part2 (of gs) -- except that with parts_shared (the fp32 matrix cores) part2 IS part.
 * NW_ERR_INVALID_ARG for a null pointer or a negative size; B <= 0: all zeros. */
#define NW_BWD_AREAS 15
typedef struct nw_bwd_plan {
    int32_t status, route;
    int32_t coeff_threads, parts_shared;
    int32_t gq_chunks, gq_k_chunk, gs_chunks, gs_k_chunk;
    int64_t ld, Bpad;
    uint64_t coeff_lds_bytes;                   /* dynamic LDS of the coefficient kernel */
    uint64_t off[NW_BWD_AREAS], bytes[NW_BWD_AREAS];
    uint64_t total;                             /* == nw_bwd_workspace_bytes(B, N, d, C, kind, sup_batched) */
} nw_bwd_plan;
int nw_debug_bwd_plan(int64_t B, int64_t N, int64_t d, int64_t C, int sup_batched, nw_bwd_plan *plan);

#ifdef __cplusplus
}
#endif
#endif /* NWHEAD_HIP_H */
