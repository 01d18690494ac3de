// Internal declarations shared by the .hip translation units of libnwhead_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/nwhead_hip.h"

#define NW_LOG_EPS 1e-12f   /* nwhead/nw.py:289 */
#define NW_NORM_EPS 1e-12f  /* F.normalize default eps, nwhead/kernel.py:19-20 */

#define NW_CHECK_LAUNCH()                          \
    do {                                           \
        if (hipGetLastError() != hipSuccess) return NW_ERR_LAUNCH; \
    } while (0)

namespace nw {

// scores (B,N) <- q (B,d), s (N,d) | (B,N,d)
int launch_scores(const float* q, const float* s, float* scores, int64_t B, int64_t N, int64_t d,
                  int kind, const float* logit_scale_dev, int sup_batched, hipStream_t st);

// softmax over supports + per-class aggregation of one (B,N) score matrix
//   final:   out (B,C), optional lse (B,), optional weights (B,N)
//   partial: m (B,), den (B,), num (B,C)
// slice_ws (nullable, slice_ws_floats): scratch of aggregate_slices(B, N) * B * (2 + C) floats -- with it, few queries over
// long rows are aggregated by several workgroups per query (partials + merge)
int aggregate_slices(int64_t B, int64_t N);
int launch_aggregate(const float* scores, const int64_t* sy, int labels_batched, float* out,
                     float* lse, float* weights, float* m, float* den, float* num, int64_t B,
                     int64_t N, int64_t C, hipStream_t st, float* slice_ws = nullptr, size_t slice_ws_floats = 0);

int launch_merge(const float* m, const float* den, const float* num, float* out, int64_t G,
                 int64_t B, int64_t C, int64_t sm, int64_t sd, int64_t sn, const int64_t* class_lo,
                 int64_t CL, hipStream_t st);

// influence.hip: softmax weights / influences from a score matrix and the forward's log-sum-exp (in place allowed)
int launch_weights_from_scores(const float* scores, const float* lse, float* weights, int64_t B, int64_t N, hipStream_t st);
int launch_influence(const float* probs_or_logp, const int64_t* qy, const float* w_or_scores, const int64_t* sy,
                     const float* lse, float* infl, int64_t B, int64_t N, int64_t C, hipStream_t st);

// squared row norms of a (rows,d) matrix (backward.hip)
int launch_rownorm2(const float* x, float* n2, int64_t rows, int64_t d, hipStream_t st);

// One area of a workspace map (FwdLayout below, BwdPlan in bwd_plan.h): byte offset from the buffer's base and size, both
// multiples of 256.
struct Area {
    size_t off, bytes;
};
inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }
// The K-split of one product of the backward: nchunks partial tiles of k_chunk each (gemm_plan in backward.hip for the
// fp32 matrix cores, xgemm_plan for the split route); chosen once per call by plan_bwd and handed to the launcher.
struct KSplit {
    int nchunks, k_chunk;
};

// bwd_split.hip: the backward's two products on the fp16 matrix cores (split-row operands)
constexpr size_t XGEMM_TAIL_BYTES = 512;   // readable bytes every operand buffer needs past its last row
KSplit xgemm_plan(int64_t M, int64_t Nn, int64_t K);
// A K-split product's reduction (out = f(m) sum_chunks part + 2 rowscale Xo), to be run by extra workgroups of a LATER
// launch_xgemm on the same stream instead of a kernel of its own (blocks == 0: nothing pending).
struct XgemmReduce {
    const float* part;
    const float* fac;
    const float* gfac;
    const float* rowscale;
    const float* Xo;
    float* out;
    int64_t M, Nn;
    int nchunks, fac_inverse, blocks;
};
int launch_xgemm(bool x_km, const float* X, int64_t ldx, int64_t x_rows, const float* Y, int64_t ldy, int64_t y_rows,
                 float* part, const float* fac, int fac_inverse, const float* gfac, const float* rowscale,
                 const float* Xo, float* out, int64_t M, int64_t Nn, int64_t K, const KSplit& p, hipStream_t st,
                 XgemmReduce* defer = nullptr, const XgemmReduce* pending = nullptr);

// bwd_query.hip: the head's gradient w.r.t. the queries over a resident split bank, no (B,N) matrix (nw_bwd_query_f32)
struct BwdQueryCall {
    const float *q, *s_split, *s_scale, *s_norm2;
    const int64_t* sy;
    const int32_t *row_lo, *row_hi;   // both or neither
    int exclude;
    const float *lse, *out, *gout;
    float *gq, *glogit_scale;
    void* workspace;
    size_t workspace_bytes;
    int64_t B, N, d, C;
    int kind;
    const float* logit_scale_dev;
    int row_chunks;
    hipStream_t st;
    const float* row_logw;   // (N,) log-weights of the bank rows (nw_bwd_query_weighted_f32), or null
    float* glogw;            // (N,) the gradient w.r.t. row_logw (nw_bwd_query_logw_f32; gq may then be null), or null
};
bool bank_head_shape_ok(int64_t N, int64_t d, int64_t C);   // capi.hip: the regime of the head over a resident bank
bool bwd_query_shape_ok(int64_t B, int64_t N, int64_t d, int64_t C);   // ... and the backward's integer ranges
size_t bwd_query_workspace_bytes(int64_t B, int64_t N, int64_t d, int64_t C, int row_chunks);
size_t bwd_logw_workspace_bytes(int64_t B, int64_t N, int64_t d, int64_t C, int row_chunks, bool want_gq);
int launch_bwd_query(const BwdQueryCall& c);

// fwd_values.hip: the value head over a resident split bank, out = softmax(scores) @ values with no (B,N) matrix
// (nw_fwd_values_f32)
struct FwdValuesCall {
    const float *q, *s_split, *s_scale, *s_norm2;
    const float *v_split, *v_scale;   // (N,T), (N,): nw_split_rows_f16x2 of the values
    const float* row_logw;            // (N,) log-weights of the bank rows, or null
    const int32_t *row_lo, *row_hi;   // both or neither
    int exclude;
    const float* lse;
    float* out;
    void* workspace;
    size_t workspace_bytes;
    int64_t B, N, d, T;
    int kind;
    const float* logit_scale_dev;
    int row_chunks;
    hipStream_t st;
};
bool fwd_values_shape_ok(int64_t B, int64_t N, int64_t d, int64_t T);   // the bank head's regime, T's, the integer ranges
size_t fwd_values_workspace_bytes(int64_t B, int64_t N, int64_t d, int64_t T, int row_chunks);
int launch_fwd_values(const FwdValuesCall& c);

// bwd_values.hip: the value head's gradient w.r.t. the queries over the same operands, no (B,N) matrix
// (nw_bwd_values_query_f32)
struct BwdValuesCall {
    const float *q, *s_split, *s_scale, *s_norm2;
    const float *v_split, *v_scale;   // (N,T), (N,): nw_split_rows_f16x2 of the values
    const float* row_logw;            // (N,) log-weights of the bank rows, or null
    const int32_t *row_lo, *row_hi;   // both or neither
    int exclude;
    const float *lse, *out, *gout;    // (B,), (B,T) the forward's raw output, (B,T) the upstream gradient
    float *gq, *glogit_scale;
    void* workspace;
    size_t workspace_bytes;
    int64_t B, N, d, T;
    int kind;
    const float* logit_scale_dev;
    int row_chunks;
    hipStream_t st;
};
bool bwd_values_shape_ok(int64_t B, int64_t N, int64_t d, int64_t T);   // fwd_values_shape_ok's regime
size_t bwd_values_workspace_bytes(int64_t B, int64_t N, int64_t d, int64_t T, int row_chunks);
int launch_bwd_values(const BwdValuesCall& c);

// bwd_values_support.hip: the value head's gradients w.r.t. the values and the row weights, contractions over the queries of
// the same recomputed weights, no (B,N) matrix (nw_bwd_values_support_f32)
struct BwdValuesSupportCall {
    const float *q, *s_split, *s_scale, *s_norm2;
    const float* v_rows;              // (N,T) the fp32 values, read for glogw only
    const float* row_logw;            // (N,) log-weights of the bank rows, or null
    const int32_t *row_lo, *row_hi;   // both or neither
    int exclude;
    const float *lse, *out, *gout;
    float *gvalues, *glogw;           // (N,T), (N,): at least one
    void* workspace;
    size_t workspace_bytes;
    int64_t B, N, d, T;
    int kind;
    const float* logit_scale_dev;
    int query_chunks;
    hipStream_t st;
};
size_t bwd_values_support_workspace_bytes(int64_t B, int64_t N, int64_t d, int64_t T, int query_chunks, bool want_gvalues);
int launch_bwd_values_support(const BwdValuesSupportCall& c);

// bwd_support.hip: the class head's gradient w.r.t. the bank rows, a contraction over the queries of the recomputed
// coefficients of bwd_query.hip, no (B,N) matrix (nw_bwd_bank_support_f32)
struct BwdBankSupportCall {
    const float *q, *s;               // (B,d) queries; (N,d) the fp32 bank rows, read for the 2 r s term only
    const float *s_split, *s_scale, *s_norm2;
    const int64_t* sy;
    const float* row_logw;            // (N,) log-weights of the bank rows, or null
    const int32_t *row_lo, *row_hi;   // both or neither
    int exclude;
    const float *lse, *out, *gout;
    float* gs;                        // (N,d)
    void* workspace;
    size_t workspace_bytes;
    int64_t B, N, d, C;
    int kind;
    const float* logit_scale_dev;
    int query_chunks;
    hipStream_t st;
};
size_t bwd_bank_support_workspace_bytes(int64_t B, int64_t N, int64_t d, int64_t C, int query_chunks);
int launch_bwd_bank_support(const BwdBankSupportCall& c);

// bwd_values_bank.hip: the value head's gradient w.r.t. the bank rows, bwd_support.hip's contraction over the queries with
// bwd_values.hip's second product in the labels' place, no (B,N) matrix (nw_bwd_values_bank_support_f32)
struct BwdValuesBankSupportCall {
    const float *q, *s;               // (B,d) queries; (N,d) the fp32 bank rows, read for the 2 r s term only
    const float *s_split, *s_scale, *s_norm2;
    const float *v_split, *v_scale;   // (N,T), (N,): nw_split_rows_f16x2 of the values
    const float* row_logw;            // (N,) log-weights of the bank rows, or null
    const int32_t *row_lo, *row_hi;   // both or neither
    int exclude;
    const float *lse, *out, *gout;    // (B,), (B,T) the forward's raw output, (B,T) the upstream gradient
    float* gs;                        // (N,d)
    void* workspace;
    size_t workspace_bytes;
    int64_t B, N, d, T;
    int kind;
    const float* logit_scale_dev;
    int query_chunks;
    hipStream_t st;
};
size_t bwd_values_bank_support_workspace_bytes(int64_t B, int64_t N, int64_t d, int64_t T, int query_chunks);
int launch_bwd_values_bank_support(const BwdValuesBankSupportCall& c);

// Options of the forward call in progress on this thread (nw_fwd_opts of the ABI, set for the duration of the call by
// the entry point): explicit arguments, not process state.
struct FwdOpts {
    const char* tables = nullptr;   // run tables of the call's labels (nw_bank_tables_build), or null
    size_t tables_bytes = 0;
    const int64_t* tables_sy = nullptr;   // ... the label array and row count they were built from
    int64_t tables_N = -1;
    int persistent_wgs = 0;         // workgroups of the persistent tile kernel (0: one per CU)
    int force_split = 0;            // split-fp16 path at every size
    int operand_form = 0;           // 0: s_split holds split rows; 1: plain fp16 rows (nw_pack_rows_f16)
};
const FwdOpts& fwd_opts();
// Diagnostic knobs (nw_debug_set; timing experiments, never needed in normal use).  KNOB_UNSET when not set.  The library
// itself never reads the environment: the Python layer forwards NW_* variables once, at load time (_lib.py).
constexpr int KNOB_UNSET = -2147483647 - 1;
enum Knob { KNOB_PVAR, KNOB_QG, KNOB_TILE_RS, KNOB_NO_PERSISTENT, KNOB_SPLIT_QUERIES, KNOB_BWD_NO_MFMA, KNOB_BWD_SPLIT,
            KNOB_XGEMM_WGS, KNOB_SPLIT_LBITS, KNOB_CONV_MAX_WGS, KNOB_CONV_SKIP_CFGS, KNOB_CONV_FORCE_CFG, KNOB_COUNT };
int knob(int id);

// fused forward (fused.hip)
int launch_topk(const float* scores, int64_t* idx, float* vals, int64_t B, int64_t N, int64_t k, hipStream_t st);  // topk.hip
// the k best of M candidates per query: keys = ordered_bits of the scores (0: empty slot), rows = their bank rows; equal
// keys must stand in ascending row order (topk.hip).  pad_empty: a query may have fewer than k candidates; a selected empty
// slot is written as row -1, value -inf, behind the valid ones
int launch_topk_candidates(const unsigned* keys, const int* rows, int64_t* idx, float* vals, int64_t B, int64_t M, int64_t k,
                           hipStream_t st, bool pad_empty = false);
// fused.hip: nearest-neighbour search over a prepared bank without the (B,N) score matrix (nw_knn_f32, nw_knn_window_f32,
// nw_knn_f16): one record for every entry point
struct KnnCall {
    const float* q;
    const void* s_rows;            // the bank's rows in `form`: split rows, or the fp16 rows of nw_pack_rows_f16
    const float *s_scale, *s_norm2;
    int64_t* idx;
    float* vals;
    void* workspace;
    size_t workspace_bytes;
    int64_t B, N, d, k;
    int kind;
    const float* logit_scale_dev;
    hipStream_t st;
    int form;                      // FORM_SPLIT or FORM_HALF (fused_plan.h)
    // both or neither: a row window per query, kept or (exclude) left out; the result is then padded with (-1, -inf).
    // FORM_SPLIT only
    const int32_t *row_lo, *row_hi;
    int exclude;
};
size_t knn_workspace_bytes(int form, int64_t B, int64_t N, int64_t d, int64_t k);
int launch_knn(const KnnCall& c);
// influence.hip: the influences of k selected supports per query (nw_influence_select_f32)
int launch_influence_select(const float* vals, const int64_t* rows, const int64_t* sy, const int64_t* qy, const float* logp,
                            const float* lse, float* infl, int64_t* labels, int64_t B, int64_t k, int64_t N, int64_t C,
                            hipStream_t st);
// knn_merge.hip: the k best of G sorted per-shard candidate lists per query, and the per-query k-NN head over them
// (nw_knn_merge_f32)
int launch_knn_merge(const float* vals, const int* rows, const int* labels, int64_t G, int64_t B, int64_t kc, int64_t stride_g,
                     int64_t k, int64_t C, int64_t* idx, float* val_out, int64_t* label_out, float* out, hipStream_t st);
int tile_timer_enable(bool on);
int tile_timer_read(double* total_us, int64_t* launches);
int pick_rs(int64_t B, int64_t N, int64_t d, bool f16 = false);
bool fused_eligible(const float* q, const float* s, int64_t B, int64_t N, int64_t d, int64_t C);
// The forward workspace of one call (nw_fwd_workspace_bytes; every forward entry point and launcher reads this record and
// nothing else), carved once, in this order: main | q_rows | q_scale | q_norm2 | lse | slices.
//   main      the (B,N) score matrix of the two-kernel path, or the fused partials (fused_layout): the larger of the two
//   q_rows, q_scale, q_norm2   the split / packed queries of a launch whose plan asks for them (FusedPlan::split_queries)
//   lse       B floats, for a call that derives weights or influences from the scores without an lse_out of its own
//   slices    the partials of the sliced aggregation, n_slices * B * (2 + C) floats; empty when n_slices == 1
// Every area starts on a multiple of 256 bytes and ends where the next one starts; the last ends at `total`.
struct FwdLayout {
    using Area = nw::Area;
    Area main, q_rows, q_scale, q_norm2, lse, slices;
    int n_slices;   // aggregate_slices(B, N), which sized `slices`
    size_t total;
    char* base;     // the caller's buffer; null: offsets and sizes only
    float* at(const Area& a) const { return base ? reinterpret_cast<float*>(base + a.off) : nullptr; }
    bool fits(size_t buffer_bytes) const { return base && buffer_bytes >= total; }   // the one workspace check of the entries
};
FwdLayout fwd_layout(int64_t B, int64_t N, int64_t d, int64_t C, void* base);   // fused.hip; B <= 0 or N <= 0: all zeros
int launch_split_rows(const float* x, float* out, float* scale, float* norm2, int64_t rows, int64_t d,
                      hipStream_t st);
// split.hip: fp32 rows -> dense fp16 rows, row scales and the norms of the ROUNDED rows (nw_pack_rows_f16)
int launch_pack_rows_f16(const float* x, void* out, float* scale, float* norm2, int64_t rows, int64_t d, hipStream_t st);
// the head on half-precision operands (nw_fwd_opts.operand_form = 1): s_rows / s_scale / s_norm2 from nw_pack_rows_f16
bool half_form_shape_ok(int64_t d);
// (the fused launch itself: launch_fused(const FusedArgs&, form, kind), fused_plan.h)

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

// Block-wide reductions for 256-thread workgroups (4 waves); `red` is >= 8 floats of LDS.
__device__ __forceinline__ float block_sum(float v, float* red) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float r = 0.f;
    const int nw_ = (blockDim.x + 63) >> 6;
    for (int w = 0; w < nw_; ++w) r += red[w];
    return r;
}
// counted wait for all but the wave's N youngest vector-memory operations; every counted wait of the library goes through
// here so that the 6-bit field is checked at compile time (an overflow once hung the test suite: DESIGN.md 4.7h)
template <int N>
__device__ __forceinline__ void wait_vmcnt() {
    static_assert(N >= 0 && N < 64, "vmcnt is a 6-bit field");
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

__device__ __forceinline__ float block_max(float v, float* red) {
    v = wave_max(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float r = -INFINITY;
    const int nw_ = (blockDim.x + 63) >> 6;
    for (int w = 0; w < nw_; ++w) r = fmaxf(r, red[w]);
    return r;
}

// exp(x) for x <= 0 in ~6 VALU instructions (libm expf is ~20; in an fp32-MFMA kernel every VALU
// instruction is matrix-pipe time).  exp(x) = 2^(x*log2e): the product is split into its rounded
// value t and its rounding error e (one FMA), 2^t comes from v_exp_f32 (<= 1 ulp) and the error is
// folded back as 2^t * (1 + e*ln2).  Relative error ~2e-7 over [-100, 0]; exact 0 for -inf.
__device__ __forceinline__ float fast_exp_neg(float x) {
    const float L2E_HI = 1.44269502162933349609375f, L2E_LO = 1.925963033500011e-8f;
    const float t = x * L2E_HI;
    const float e = __builtin_fmaf(x, L2E_HI, -t) + x * L2E_LO;
    const float r = __builtin_amdgcn_exp2f(t);
    return (x == -INFINITY) ? 0.f : __builtin_fmaf(r * e, 0.693147182464599609375f, r);
}

// sqrt(max(x,0)) with the hardware v_sqrt_f32 (<= 1 ulp) instead of the ~12-instruction correctly
// rounded sequence; x is a squared distance, 1 ulp of its root is below the fp32 spacing the
// reference's own result has.
__device__ __forceinline__ float fast_sqrt_pos(float x) { return __builtin_amdgcn_sqrtf(fmaxf(x, 0.f)); }

// Reductions over the four lanes {i, i+16, i+32, i+48} of a wave (the four k-groups of a 16x16 MFMA
// accumulator column), result in all four.  gfx950's v_permlane{32,16}_swap are plain VALU ops
// (mov + swap + op = 3 issue slots per step); __shfl_xor goes through ds_bpermute and its LDS round
// trip (~120 cycles per step, exposed when one wave per SIMD runs an epilogue).
__device__ __forceinline__ float group4_sum(float x) {
    typedef unsigned u2_ __attribute__((ext_vector_type(2)));
    u2_ r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    x = __uint_as_float(r[0]) + __uint_as_float(r[1]);
    r = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
__device__ __forceinline__ float group4_min(float x);
__device__ __forceinline__ float group4_max(float x) {
    typedef unsigned u2_ __attribute__((ext_vector_type(2)));
    u2_ r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    x = fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
    r = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}

__device__ __forceinline__ float group4_min(float x) {
    typedef unsigned u2_ __attribute__((ext_vector_type(2)));
    u2_ r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    x = fminf(__uint_as_float(r[0]), __uint_as_float(r[1]));
    r = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return fminf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}

// group4_sum / group4_min / group4_max of NV independent values at once (op = the two-input add / min / max): per value the
// same two steps on the same operands, but the swaps of all values are issued together, so that the VALU-write -> permlane
// hazard padding and the swap latency of one value lie under the others' instructions.
template <int NV, typename Op>
__device__ __forceinline__ void group4_each(float (&v)[NV], Op op) {
    typedef unsigned u2_ __attribute__((ext_vector_type(2)));
    u2_ r[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) r[k] = __builtin_amdgcn_permlane32_swap(__float_as_uint(v[k]), __float_as_uint(v[k]), false, false);
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] = op(__uint_as_float(r[k][0]), __uint_as_float(r[k][1]));
#pragma unroll
    for (int k = 0; k < NV; ++k) r[k] = __builtin_amdgcn_permlane16_swap(__float_as_uint(v[k]), __float_as_uint(v[k]), false, false);
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] = op(__uint_as_float(r[k][0]), __uint_as_float(r[k][1]));
}

// group4_max / group4_min of unsigned values (the candidate selection of the tile epilogue works on ordered_bits keys)
__device__ __forceinline__ unsigned group4_max_u32(unsigned x) {
    typedef unsigned u2_ __attribute__((ext_vector_type(2)));
    u2_ r = __builtin_amdgcn_permlane32_swap(x, x, false, false);
    x = max(r[0], r[1]);
    r = __builtin_amdgcn_permlane16_swap(x, x, false, false);
    return max(r[0], r[1]);
}
__device__ __forceinline__ unsigned group4_min_u32(unsigned x) {
    typedef unsigned u2_ __attribute__((ext_vector_type(2)));
    u2_ r = __builtin_amdgcn_permlane32_swap(x, x, false, false);
    x = min(r[0], r[1]);
    r = __builtin_amdgcn_permlane16_swap(x, x, false, false);
    return min(r[0], r[1]);
}

// Order-preserving uint image of a float: larger float <=> larger uint, NaN on top.  0 is the image of no float (the
// smallest, -inf, is 0x007fffff): the selection kernels use it for "not an element".
__device__ __forceinline__ unsigned ordered_bits(float f) {
    unsigned b = __float_as_uint(f);
    if ((b & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;  // every NaN, either sign: one image above +inf (torch's order)
    if ((b << 1) == 0) b = 0;  // -0.0 == +0.0: one image, so that their order is the index order
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
// ... and back (the NaN image gives a quiet NaN, the one image of the zeros +0.0)
__device__ __forceinline__ float ordered_bits_to_float(unsigned u) {
    return __uint_as_float((u & 0x80000000u) ? (u ^ 0x80000000u) : ~u);
}

// score from (dot, |q|^2, |s|^2); shared by the MFMA and the generic kernels
template <int KIND>
__device__ __forceinline__ float score_from_dot(float dot, float qn2, float sn2, float scale) {
    if (KIND == NW_SCORE_DOT) return dot;
    if (KIND == NW_SCORE_EUCLIDEAN) return -fast_sqrt_pos(qn2 + sn2 - 2.f * dot);
    const float nq = fmaxf(sqrtf(qn2), NW_NORM_EPS), ns = fmaxf(sqrtf(sn2), NW_NORM_EPS);
    const float c = dot / (nq * ns);
    if (KIND == NW_SCORE_COSINE) return c;
    if (KIND == NW_SCORE_CLIP) return scale * c;
    // hypersphere: -||x/|x| - y/|y|||, matmul form like torch's cdist for N > 25
    const float a = qn2 / (nq * nq), b = sn2 / (ns * ns);
    return -fast_sqrt_pos(a + b - 2.f * c);
}


// The same scores, factored for the tile epilogues: with per-support-row factors (K, Base), per-query
// factors (Cq, Bq) and x = acc * K * Cq + (Base + Bq), the score in BASE-2 units (u = score * log2 e) is
// finish(x).  `acc` is the raw accumulator (for split-fp16 operands the dot product times 2^(e_q + e_s);
// sscale / qscale = 2^-e of the row, 1 for fp32 operands).  Everything that depends on one row only --
// square roots, reciprocals, the normalisation of the cosine-type kernels -- is done once per row here
// instead of once per (query, support) pair; 1/x is v_rcp_f32 (1 ulp), well inside the 1e-5 bar.
template <int KIND>
struct ScoreFactors {
    static constexpr float L2E = 1.44269504088896340736f;
    static constexpr bool DIST = (KIND == NW_SCORE_EUCLIDEAN || KIND == NW_SCORE_HYPERSPHERE);
    static constexpr bool NORMALISED = (KIND == NW_SCORE_HYPERSPHERE || KIND == NW_SCORE_COSINE || KIND == NW_SCORE_CLIP);
    static __device__ __forceinline__ float inv_norm(float n2) {  // 1 / max(|x|, eps), F.normalize's eps
        return __builtin_amdgcn_rcpf(fmaxf(__builtin_amdgcn_sqrtf(n2), NW_NORM_EPS));
    }
    static __device__ __forceinline__ void support(float n2, float sscale, float& K, float& Base) {
        const float in = NORMALISED ? inv_norm(n2) : 1.f;
        K = sscale * in * (DIST ? -2.f * L2E * L2E : L2E);
        Base = DIST ? (NORMALISED ? n2 * in * in : n2) * (L2E * L2E) : 0.f;
    }
    // support() in parts, every product rounded on its own, for a kernel that makes a row's factors once and finishes
    // Base + Bq elsewhere (fused_f16p12.h): K as support() makes it, t = Base's norm term, Bp = Base = t * L2E^2 rounded.
    // Whoever adds Bq chooses fma(t, L2E^2, Bq) or Bp + Bq (base_plus below: the two differ in the last bit).
    static __device__ __forceinline__ void support_parts(float n2, float sscale, float& K, float& t, float& Bp) {
        const float in = NORMALISED ? inv_norm(n2) : 1.f;
        K = __fmul_rn(__fmul_rn(sscale, in), DIST ? -2.f * L2E * L2E : L2E);
        t = DIST ? (NORMALISED ? __fmul_rn(__fmul_rn(n2, in), in) : n2) : 0.f;
        Bp = DIST ? __fmul_rn(t, L2E * L2E) : 0.f;
    }
    static __device__ __forceinline__ void query(float n2, float qscale, float clip_scale, float& Cq, float& Bq) {
        const float in = NORMALISED ? inv_norm(n2) : 1.f;
        Cq = qscale * in * (KIND == NW_SCORE_CLIP ? clip_scale : 1.f);
        Bq = DIST ? (NORMALISED ? n2 * in * in : n2) * (L2E * L2E) : 0.f;
    }
    // Base + Bq of support() / query() with its roundings spelled out instead of left to the compiler's contraction: one
    // fused multiply-add, or (`separate`) the product and the sum rounded on their own.  For a kernel that has to return
    // another kernel's bits (fused_impl.h, OUT_CAND_WIN).
    static __device__ __forceinline__ float base_plus(float n2, float Bq, bool separate) {
        if (!DIST) return 0.f;
        const float in = NORMALISED ? inv_norm(n2) : 1.f;
        const float t = NORMALISED ? n2 * in * in : n2;
        return separate ? __fadd_rn(__fmul_rn(t, L2E * L2E), Bq) : __builtin_fmaf(t, L2E * L2E, Bq);
    }
    static __device__ __forceinline__ float finish(float x) { return DIST ? -fast_sqrt_pos(x) : x; }
    // the same without the sign for the distance kernels (u = -finish_abs(x)): the persistent epilogue
    // carries distances and takes their MINIMUM, which saves one negation per pair
    static __device__ __forceinline__ float finish_abs(float x) { return DIST ? fast_sqrt_pos(x) : x; }
};

}  // namespace nw
