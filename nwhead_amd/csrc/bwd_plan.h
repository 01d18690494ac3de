// bwd_plan.h -- the head's backward as a value: route, coefficient launch, K-splits and workspace map of one call
// (BwdPlan, made by plan_bwd in backward.hip).  nw_bwd_workspace_bytes, nw_bwd_uses_split, nw_debug_bwd_plan and the
// launcher nw_bwd_bank_f32 read this record and nothing else.
#pragma once
#include "nw_internal.h"

namespace nw {

// The route of the two products gq = A s + 2 rq q and gs = A^T q + 2 rs s:
//   BWD_VALU   plain VALU kernels: per-query supports, rows that are no whole float4s, too little work for the chip
//   BWD_MFMA   fp32 matrix cores (nw_bwd_gemm_kernel): shared supports, d % 4 == 0, B N d >= BWD_MFMA_MIN_WORK
//   BWD_SPLIT  fp16 matrix cores on split rows (bwd_split.hip): the above and d % 32 == 0, the coefficient kernel's LDS
//              within BWD_SPLIT_LDS_CAP, B >= BWD_SPLIT_MIN_B and N >= BWD_SPLIT_MIN_N
// Knobs: bwd_no_mfma = 1 leaves only BWD_VALU; bwd_split = 0 never splits, = 1 lifts the B and N thresholds (nothing else).
enum BwdRoute { BWD_VALU = 0, BWD_MFMA = 1, BWD_SPLIT = 2 };

constexpr int64_t BWD_MFMA_MIN_WORK = (int64_t)1 << 22;   // B N d from which the products fill the chip's matrix cores
// The extra passes of the split route (splitting the supports and the queries) have to pay: with B N d >= 2^22 it is ahead
// at every shape measured from these sizes (tools/bwd_crossover.py); at B=256, N=10000, d=512 the backward's kernels take
// 64 us against 157 on the fp32 cores.
constexpr int64_t BWD_SPLIT_MIN_B = 16, BWD_SPLIT_MIN_N = 256;

// Dynamic LDS of nw_bwd_coeff_kernel: BWD_COEFF_LDS_FIXED floats of reduction scratch (16 for block_sum, 64 for the
// combined four-value round), the C class gradients dP, and on the split route one staged row of A (ld floats).
constexpr int64_t BWD_COEFF_LDS_FIXED = 80;
// The launcher's cap, a CU's 160 KiB of LDS: past it NW_ERR_UNSUPPORTED (with 80 + C floats: C = 40880 is the last class
// count the backward takes).  No launch site sets hipFuncAttributeMaxDynamicSharedMemorySize: this runtime needs none.
constexpr size_t BWD_COEFF_LDS_CAP = 160 * 1024;
// The split route's cap: 80 + ld + C <= 38400 floats (C = 16: N = 38300 splits, N = 38305 runs the fp32 matrix cores).
constexpr size_t BWD_SPLIT_LDS_CAP = 150 * 1024;
inline size_t bwd_coeff_lds_bytes(int64_t C, int64_t staged_row) {
    return (size_t)(BWD_COEFF_LDS_FIXED + C + staged_row) * sizeof(float);
}
// One workgroup per query: 256 threads, 1024 from this row length.
constexpr int64_t BWD_COEFF_WIDE_N = 2048;
inline unsigned bwd_coeff_threads(int64_t N) { return N >= BWD_COEFF_WIDE_N ? 1024 : 256; }

// The workspace (nw_bwd_workspace_bytes), carved once, in this order; every area starts on a multiple of 256 bytes where
// the one before ends, an area its route does not use is empty, the last ends at `total`.
//   A        (B, ld) coefficients; on the split route their split-row image, + XGEMM_TAIL_BYTES
//   RS_PAIR  (B, ld) per-pair norm coefficients Rs
//   RQ, GLS, QN2   B floats each: the queries' norm coefficient, logit-scale gradient terms, squared norms
//   SN2      the supports' squared norms: N floats, B N with per-query supports
//   RS       N floats: column sums of RS_PAIR (both matrix-core routes)
//   S_SPLIT, S_SCALE   split route: the supports as split rows (N d floats + tail) and their N row scales; reserved
//            even when the caller's bank is read instead
//   Q_SPLIT  split route: q'' as split rows, Bpad rows (B rounded up to 32, the rest zero) + tail
//   ASCALE, QV, GFAC   split route: 2^-E_b and max|q_b| 2^-E_b per query, and the batch factor 2^-G
//   PART     partial tiles of the first product (gq), cq B d floats when cq > 1
//   PART2    ... of the second (gs), cs N d floats when cs > 1.  Split route: an area of its own, because the first
//            product's tiles are still pending while the second runs.  fp32 matrix cores: THE SAME area as PART
//            (parts_shared), sized for the larger of the two.
enum BwdArea { BWD_A, BWD_RS_PAIR, BWD_RQ, BWD_GLS, BWD_QN2, BWD_SN2, BWD_RS, BWD_S_SPLIT, BWD_S_SCALE, BWD_Q_SPLIT,
               BWD_ASCALE, BWD_QV, BWD_GFAC, BWD_PART, BWD_PART2, BWD_AREAS };

struct BwdPlan {
    int status;             // NW_OK, or NW_ERR_UNSUPPORTED: the coefficient kernel's LDS exceeds BWD_COEFF_LDS_CAP
    int route;              // BwdRoute
    int64_t ld;             // row stride of A and RS_PAIR: N, N rounded up to 4 floats (BWD_MFMA) or to 32 (BWD_SPLIT)
    int64_t Bpad;           // rows of Q_SPLIT
    unsigned coeff_threads;
    size_t coeff_lds;
    KSplit gq, gs;          // K-split of the two products (gemm_plan / xgemm_plan); zero on BWD_VALU
    Area area[BWD_AREAS];
    bool parts_shared;
    size_t total;
    char* base;             // the caller's buffer; null: offsets and sizes only
    float* at(int a) const { return base ? reinterpret_cast<float*>(base + area[a].off) : nullptr; }
    bool fits(size_t buffer_bytes) const { return base && buffer_bytes >= total; }
};
// backward.hip; reads the knobs bwd_no_mfma, bwd_split and xgemm_wgs.  B <= 0 or N < 0: all zeros.
BwdPlan plan_bwd(int64_t B, int64_t N, int64_t d, int64_t C, int sup_batched, void* base = nullptr);

}  // namespace nw
