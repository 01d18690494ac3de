// fused_plan.h -- the launch decision of the fused head as a value (FusedPlan, made by plan_fused in fused.hip) and the
// argument record its launchers take (FusedArgs).  Shared by fused.hip, fused_impl.h and capi.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace nw {

struct FwdOpts;
struct FwdLayout;
struct CandOut;
#define NW_FOR_EACH_KIND(X) \
    X(NW_SCORE_EUCLIDEAN) X(NW_SCORE_HYPERSPHERE) X(NW_SCORE_COSINE) X(NW_SCORE_DOT) X(NW_SCORE_CLIP)

// MODE_REG : register-staged loaders (tile_core.h), any d % 4 == 0; loaders compute both norms
// MODE_DMA : LDS-DMA loaders (tile_dma.h), d % 32 == 0; consumers compute both norms
// MODE_DMA_SN : LDS-DMA loaders, support norms supplied by the caller (cached bank)
// MODE_F16 : LDS-DMA loaders, split-fp16 operands on the fp16 matrix cores (tile_f16.h): q and s are
//            SPLIT rows, norms and row scales of both are supplied
// MODE_F16Q: as MODE_F16, but q holds the caller's RAW fp32 rows: the consumer waves compute the row scales and
//            norms in their prologue and split their query fragments in registers (tile_f16.h, QRAW) -- the
//            one-workgroup-per-tile kernel of small grids (T) runs without a query-split launch in front
//   (Measured and dropped, T shape: the query fragments RESIDENT in the consumer waves -- high halves in 64 VGPRs, low
//    halves parked in LDS, only support rows in the stage ring, one set of support fragments refilled block by block.
//    29 % fewer bytes through the loop's L2 -> LDS stream, but getting the rows into operand shape cost 11.5 k cycles
//    per workgroup (fragment-shaped global loads, or sixteen 8 KB DMA steps each paying a third of the DMA latency)
//    and the single-buffered loop ran 750 cycles per stage against 530: 18.5-19.4 us against 16.4.)
enum { MODE_REG = 0, MODE_DMA = 1, MODE_DMA_SN = 2, MODE_F16 = 3, MODE_F16Q = 4 };
constexpr bool mode_is_f16(int m) { return m == MODE_F16 || m == MODE_F16Q; }
// What a tile leaves behind besides (OUT_NONE, OUT_SCORES) or instead of (OUT_CAND) its softmax partials: nothing, its
// block of the (B,N) score matrix, or its best k scores per query (CandOut; split or half-precision operands, no labels, no merge).
// OUT_WIN: the softmax partials of OUT_NONE over the bank rows that a per-query row window admits (FusedArgs::win_lo / win_hi,
// nw_fwd_window_f32; split operands on nw_fused_kernel only, never the persistent kernels).  (3 is OUT_CAND_WIN, fused_impl.h.)
// OUT_WGT: OUT_WIN with a log-weight per bank row added to the scores (FusedArgs::row_logw, nw_fwd_weighted_f32); the window
// is optional there.  Same operands, kernels and plans as OUT_WIN.
enum { OUT_NONE = 0, OUT_SCORES = 1, OUT_CAND = 2, OUT_WIN = 4, OUT_WGT = 5 };
constexpr bool out_is_win(int out) { return out == OUT_WIN || out == OUT_WGT; }
// The support operand: fp32 rows, split rows (nw_split_rows_f16x2) or half-precision rows (nw_pack_rows_f16).
enum { FORM_F32 = 0, FORM_SPLIT = 1, FORM_HALF = 2 };

struct FusedPlan {
    int form;                    // FORM_* of the support operand
    int status;                  // NW_OK, or what the launcher returns for this combination (nothing is launched then)
    int rs, BS, n_stiles;        // support tile: height in 16-row blocks, rows, tiles over the bank
    int n_qtiles, grid;          // 64-query tiles; workgroups of the one-workgroup-per-tile kernel (padded_grid)
    int mode, out;               // MODE_* / OUT_* of nw_fused_kernel (persistent: the form of its operands)
    bool dma;                    // LDS-DMA loaders possible (d % 32 == 0, tile-relative offsets fit)
    bool persistent;             // nw_fused_f16p_kernel / nw_fused_f16p_kernel_w12 instead of nw_fused_kernel
    bool split_queries;          // a split (FORM_SPLIT) or pack (FORM_HALF) launch of the queries precedes the tile kernel
    bool run_tables;             // the tile kernel reads run tables: the bank's (bank_tables_take) or built by the launch
    int variant, workgroups, qgroup;   // persistent only: tile variant 0-3, grid, query tiles kept resident per XCD
    size_t lds_bytes;            // dynamic LDS of the tile kernel
};
// Tile geometry alone (rs .. grid): all that the workspace layouts depend on.  No CU count, no knob but tile_rs.
FusedPlan plan_tiles(int64_t B, int64_t N, int64_t d, int form);
// The whole decision.  out: OUT_* (k: OUT_CAND's candidates per query); norms: support norms supplied; cus: CU count,
// 0 = the device's.  The diagnostic knobs of the fused path are read here and nowhere else.
FusedPlan plan_fused(int64_t B, int64_t N, int64_t d, int64_t C, int form, int out, int k, bool norms, bool dot, int cus,
                     const FwdOpts& opts);

// One forward call's operands, as the launchers take them.  out != nullptr: final log-probabilities (+ optional scores /
// lse); out == nullptr: the partials (m, den, num); cand != nullptr: candidates instead of either (nw_knn_f32, nw_knn_f16).
struct FusedArgs {
    const float* q;              // the caller's RAW fp32 queries
    const float* s;              // support rows in the plan's form (FORM_HALF: fp16 rows behind a float pointer)
    const int64_t* sy;
    const float *s_norm2, *s_scale, *ls;
    float *out, *scores, *lse, *m, *den, *num;
    const FwdLayout* ws;         // the call's workspace, carved and checked by the entry point (nw_internal.h); null with cand
    int B, N, d, C;
    hipStream_t st;
    const CandOut* cand;
    const int *win_lo, *win_hi;
    int win_exclude;
    const float* row_logw;       // (N,) natural-log weight of every bank row (OUT_WGT), or null
};
int launch_fused(const FusedArgs& a, int form, int kind);   // plan_fused + the launcher of the score kind (fused.hip)

}  // namespace nw
