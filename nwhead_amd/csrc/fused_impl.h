// fused_impl.h -- nw_fused_kernel and its per-score-kind launcher (gfx950 / MI355X only).
// Included by fused_k*.hip, one translation unit per score kind so that the build parallelises.
#pragma once
#include <type_traits>
#include "tile_core.h"
#include "tile_dma.h"
#include "tile_f16.h"
#include "fused_plan.h"

namespace nw {

constexpr int RUN_CAP = 192;  // >= 16*RS for the largest RS

struct FusedWs {  // views into the caller's workspace
    float* m;     // [n_stiles][B]
    float* den;   // [n_stiles][B]
    int* nrun;    // [n_stiles]
    int* lab;     // [n_stiles][BS]      label of run r (-1: padding / out-of-range label)
    float* num;   // [n_stiles][BS][B]   run sums, rows >= nrun[st] never touched
    int* runid;   // [n_stiles][BS] (+64)  run of every support row inside its tile (persistent kernel only)
    int* bnd;     // [n_stiles][2]  first tile rows of runs 1 and 2 (BS when there is no such run)
    int* ctab;    // [C][3 + MENT]  the run merge's class tables when they do not fit in LDS (nw_class_tables_kernel)
};
size_t fused_layout(int64_t B, int64_t n_stiles, int BS, char* base, FusedWs* ws, int64_t C = 0);
int launch_run_tables(const FusedWs& ws, const int64_t* sy, int N, int C, int n_stiles, int BS, hipStream_t st);
bool bank_tables_take(const int64_t* sy, int N, int C, int n_stiles, int BS, FusedWs* ws);   // the caller's cached tables, if named for this call
int launch_merge_runs(const FusedWs& ws, float* out, float* lse, float* m, float* den, float* num,
                      int B, int C, int n_stiles, int BS, hipStream_t st);
// Candidate output of the tile kernel (nw_knn_f32): instead of softmax partials every (query, support tile) pair leaves
// its kc = min(k, tile rows) best scores, best first, ties in ascending bank-row order, as ordered_bits keys (0: empty slot)
// and bank rows: key / row [b][st][j], j < kcp = kc rounded up to 4.  q_rows / q_scale / q_norm2: room for the split form
// of the queries when the launch decision asks for the split launch.
// win_lo / win_hi (nw_knn_window_f32; null: no window): per query the bank rows [lo, hi) that may be candidates, or,
// with win_exclude, the rows that may not.  The kernel clamps both to [0, N] and never uses them as addresses.
struct CandOut {
    unsigned* key;
    int* row;
    int k;
    float *q_rows, *q_scale, *q_norm2;
    const int *win_lo, *win_hi;
    int win_exclude;
};
constexpr int CAND_EXCLUDE = 1 << 8;   // the flag's place beside k (<= 32) in the kernel's k argument; set only with a window
// nw_fused_kernel's OUT for the candidate output WITH a row window.  A template argument only (plans say OUT_CAND): the
// kernels without a window are compiled from the text they always had, so nw_knn_f32's code and bits do not move.
constexpr int OUT_CAND_WIN = 3;
constexpr bool out_is_cand(int out) { return out == OUT_CAND || out == OUT_CAND_WIN; }
// Softmax partials over a per-query row window (OUT_WIN, nw_fwd_window_f32).  The window is applied to the scores before the
// tile maximum, so a (query, tile) pair may keep no row: a DEAD pair.  Its tile stores m = -inf, den = 0 and 0 in every run
// sum below the tile's run count -- all the run merge reads of it (the workspace is never cleared) -- and the merge gives a
// query whose every pair is dead log(NW_LOG_EPS) in every class and lse = -inf (nw_merge_runs_kernel).
// The kernel's arguments stay those of every other output: the window's two arrays (read only) stand where the scores and
// the tile sums go, the flag beside the class count (< 2^30, fused_eligible); the kernel finds the tile sums behind the tile
// maxima, where fused_layout puts them.
constexpr int WIN_EXCLUDE = 1 << 30;
__host__ __device__ inline size_t fused_den_after_m(int64_t n_stiles, int64_t B) {   // floats from FusedWs::m to FusedWs::den
    return (((size_t)n_stiles * (size_t)B * 4 + 255) & ~(size_t)255) / 4;
}
__host__ __device__ inline int cand_slots(int k, int BS) { return ((k < BS ? k : BS) + 3) & ~3; }
int tile_timer_start(hipStream_t st);          // diagnostics (nw_debug_tile_timing): -1 when disabled
void tile_timer_stop(int slot, hipStream_t st);

namespace {

// Runs of equal consecutive labels inside one support tile, by ONE wave (3 rows per lane): fills
// runid[t] (run of tile row t), runlab[run] (its class, -1 = padding / out-of-range label), nrun_s[0] =
// number of runs and nrun_s[1], nrun_s[2] = first tile rows of runs 1 and 2 (BS when there is none).
// `lab` = this lane's three labels (tile rows 3*lane .. 3*lane+2), already mapped to -1 when invalid.
template <int BS>
__device__ __forceinline__ void run_scan_wave(const int (&lab)[3], int lane, int* runid, int* runlab, int* nrun_s) {
    int flag[3];
    if (lane < 2) nrun_s[1 + lane] = BS;  // overwritten below by the lane that starts run 1 / run 2 (same wave: in order)
    const int prev_last = __shfl_up(lab[2], 1);
    flag[0] = (lane == 0) || (lab[0] != prev_last);
    flag[1] = lab[1] != lab[0];
    flag[2] = lab[2] != lab[1];
    int incl = flag[0] + flag[1] + flag[2];
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(incl, o);
        if (lane >= o) incl += v;
    }
    int id = incl - (flag[0] + flag[1] + flag[2]) - 1;  // run id before this lane's rows
#pragma unroll
    for (int u = 0; u < 3; ++u) {
        const int t = 3 * lane + u;
        id += flag[u];
        if (t < BS) {
            runid[t] = id;
            if (flag[u] && (id == 1 || id == 2)) nrun_s[id] = t;
            if (flag[u]) runlab[id] = lab[u];
            if (t == BS - 1) *nrun_s = id + 1;
        }
    }
}
template <int BS>
__device__ __forceinline__ void load_tile_labels(const int64_t* __restrict__ sy, int s0, int N, int C, int lane, int (&lab)[3]) {
#pragma unroll
    for (int u = 0; u < 3; ++u) {
        const int t = 3 * lane + u, j = s0 + t;
        int64_t y = -1;
        if (t < BS && j < N) y = sy[j];
        lab[u] = ((uint64_t)y < (uint64_t)C) ? (int)y : -1;
    }
}

// OUT_CAND: the tile's kc best scores of every query column, selected from the registers of the epilogue.  A query column
// is the four lanes g = 0..3 (lanes i, i+16, i+32, i+48), lane (i, g) holding tile rows 16r + 4g + e.  The keys are
// ordered_bits of the floats the score writer WOULD store (sc * ln2: the product is only weakly monotone in sc, so
// selecting on sc would break a rounding tie differently), rows past the bank are 0 = "no element".  One round per
// candidate: in-lane maximum, maximum over the four lanes, the LOWEST tile row among the keys equal to it (in-lane first,
// then over the lanes), knock that one element out.  Four rounds fill one slot in each of the column's four lanes, which
// the whole wave then stores at once (16 bytes per query).
// WIN: win_lo / win_hi hold a row window per query.  Keys of rows that the window does not admit become "no element" as
// well; k then carries CAND_EXCLUDE.  A (query column, tile) pair that the window leaves whole skips the per-key
// comparisons, as a tile that does not reach N does above, and a wave none of whose columns keeps a row stores its empty
// slots without running the selection.
template <int RS, bool WIN = false>
__device__ __forceinline__ void tile_candidates(const float (&sc)[RS][4], unsigned* __restrict__ cand_key,
                                                int* __restrict__ cand_row, int B, int N, int b, int s0, int g, int st,
                                                int n_stiles, int k, const int* __restrict__ win_lo = nullptr,
                                                const int* __restrict__ win_hi = nullptr) {
    constexpr int BS = 16 * RS;
    constexpr float LN2 = 0.693147180559945309417f;
    constexpr unsigned NOPOS = 1u << 20;
    unsigned key[RS][4];
#pragma unroll
    for (int r = 0; r < RS; ++r)
#pragma unroll
        for (int e = 0; e < 4; ++e) key[r][e] = ordered_bits(sc[r][e] * LN2);
    if (s0 + BS > N) {
#pragma unroll
        for (int r = 0; r < RS; ++r)
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (s0 + 16 * r + 4 * g + e >= N) key[r][e] = 0u;
    }
    bool dead = false;   // (window only) this query keeps no row of the tile
    if constexpr (WIN) {
        const bool exclude = (k & CAND_EXCLUDE) != 0;
        k &= CAND_EXCLUDE - 1;
        const int bb = b < B ? b : B - 1;
        const int lo = min(max(win_lo[bb], 0), N), hi = min(max(win_hi[bb], 0), N);
        const unsigned width = hi > lo ? (unsigned)(hi - lo) : 0u;
        const int tile_end = s0 + BS < N ? s0 + BS : N;
        const bool disjoint = width == 0u || hi <= s0 || lo >= tile_end;   // no row of the tile is in the window
        const bool covered = lo <= s0 && hi >= tile_end;                    // every row of the tile is
        dead = exclude ? covered : disjoint;
        if (!(exclude ? disjoint : covered)) {
            const int rel = s0 + 4 * g - lo;   // tile row t = 16r + e of this lane is bank row lo + rel + t
#pragma unroll
            for (int r = 0; r < RS; ++r)
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (((unsigned)(rel + 16 * r + e) < width) == exclude) key[r][e] = 0u;
        }
    }
    const int kc = k < BS ? k : BS, kcp = cand_slots(k, BS);
    const size_t base = ((size_t)b * n_stiles + st) * kcp + g;
    if (WIN && __all(dead)) {
        for (int j0 = 0; j0 < kcp; j0 += 4)
            if (b < B) {
                cand_key[base + j0] = 0u;
                cand_row[base + j0] = s0;
            }
        return;
    }
    for (int j0 = 0; j0 < kcp; j0 += 4) {
        unsigned okey = 0u;
        int orow = 0;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (j0 + u >= kc) break;  // (the same for every lane)
            unsigned m = 0u;
#pragma unroll
            for (int r = 0; r < RS; ++r) m = max(max(m, key[r][0]), max(key[r][1], max(key[r][2], key[r][3])));
            m = group4_max_u32(m);
            unsigned pos = NOPOS;   // 16r + e of this lane's lowest row holding m
#pragma unroll
            for (int r = RS - 1; r >= 0; --r)
#pragma unroll
                for (int e = 3; e >= 0; --e) pos = key[r][e] == m ? (unsigned)(16 * r + e) : pos;
            const unsigned win = group4_min_u32(pos + 4u * g);   // tile row of the winner (every key 0: some empty row)
            const unsigned mine = win - 4u * g;
#pragma unroll
            for (int r = 0; r < RS; ++r)
#pragma unroll
                for (int e = 0; e < 4; ++e) key[r][e] = (unsigned)(16 * r + e) == mine ? 0u : key[r][e];
            if (g == u) {
                okey = m;
                orow = s0 + (int)win;
            }
        }
        if (b < B) {
            cand_key[base + j0] = okey;
            cand_row[base + j0] = orow;
        }
    }
}

// The head's row window on the scores of one tile (OUT_WIN, OUT_WGT): tile_candidates<RS, true>'s window arithmetic.  Rows
// that the query's window does not admit leave the softmax like the rows past the bank.  A (query column, tile) pair that the
// window leaves whole skips the per-element comparisons; lo / hi are clamped and never used as addresses.
template <int RS>
__device__ __forceinline__ void window_scores(float (&sc)[RS][4], const int* __restrict__ win_lo, const int* __restrict__ win_hi,
                                              bool exclude, int b, int B, int N, int s0, int g) {
    constexpr int BS = 16 * RS;
    const int bb = b < B ? b : B - 1;
    const int lo = min(max(win_lo[bb], 0), N), hi = min(max(win_hi[bb], 0), N);
    const unsigned width = hi > lo ? (unsigned)(hi - lo) : 0u;
    const int tile_end = s0 + BS < N ? s0 + BS : N;
    const bool disjoint = width == 0u || hi <= s0 || lo >= tile_end;   // no row of the tile is in the window
    const bool covered = lo <= s0 && hi >= tile_end;                    // every row of the tile is
    if (!(exclude ? disjoint : covered)) {
        const int rel = s0 + 4 * g - lo;   // tile row t = 16r + e of this lane is bank row lo + rel + t
#pragma unroll
        for (int r = 0; r < RS; ++r)
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (((unsigned)(rel + 16 * r + e) < width) == exclude) sc[r][e] = -INFINITY;
    }
}

#ifdef NW_DIAG_FUSED   // diagnostic build only (tools/bench_fused.hip): phase stamps go to `scores`
#define NW_FSTAMP(k) if (threadIdx.x == 0) reinterpret_cast<unsigned long long*>(scores)[8 * blockIdx.x + (k)] = __builtin_amdgcn_s_memtime()
#else
#define NW_FSTAMP(k)
#endif
// The epilogue of one tile: scores -> tile-local softmax statistics -> run sums -> workspace.
// Called by all threads of the workgroup (loader waves only take part in the run-table copy).
// OUT_CAND: `scores` / `ws_lab` are CandOut's key / row arrays, n_stiles and k come behind; nothing else is written.
// OUT_CAND_WIN: `ws_nrun` / `ws_m` are CandOut's window arrays besides, loaded in tile_candidates.
// OUT_WIN: `scores` / `ws_den` are the row window's two arrays (the tile sums go to ws_m + fused_den_after_m), k carries
// the kernel's C argument (WIN_EXCLUDE); everything else as for OUT_NONE.
// OUT_WGT: OUT_WIN with `row_logw` (N natural-log weights of the bank rows, read from global memory here, behind the main
// loop: no register is held across it and the LDS header stays what it is); the window's arrays may both be null.
template <int RS, int KIND, int OUT, int MODE>
__device__ __forceinline__ void fused_epilogue(
    f32x4 (&acc)[RS], const float* qn2, const float* sn2, const float* ssc, const int* runid,
    const int* runlab, const int* nrun_s, const float* qsc_s,
    const float* __restrict__ logit_scale, float* __restrict__ scores, float* __restrict__ ws_m,
    float* __restrict__ ws_den, int* __restrict__ ws_nrun, int* __restrict__ ws_lab,
    float* __restrict__ ws_num, int B, int N, int q0, int s0, int qt, int st, int n_stiles = 0, int k = 0,
    const float* __restrict__ row_logw = nullptr) {
    constexpr int BS = 16 * RS;
    constexpr bool WRITE_SCORES = OUT == OUT_SCORES;
    constexpr bool NEED_NORM = (KIND != NW_SCORE_DOT);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int i = lane & 15, g = lane >> 4;
    const bool consumer = wave < NCONS;  // waves 4-7 (loaders) hold no accumulators
    // The softmax part works in BASE-2 units u = score * log2(e): e^(s-m) = 2^(u-mu) is then one
    // subtract and one v_exp_f32, and for the Euclidean kernel the constant is folded into the
    // squared distance (u = -sqrt(log2(e)^2 * d2)), so an element costs fma, fma, max, sqrt, sub,
    // exp2 + its share of the reductions -- in an fp32-MFMA kernel every VALU instruction is
    // matrix-pipe time.  Tile statistics (ws_m) are kept in base-2 units; the merge converts.
    constexpr float L2E = 1.44269504088896340736f, LN2 = 0.693147180559945309417f;
    float scale = 1.f;
    if (KIND == NW_SCORE_CLIP) scale = expf(*logit_scale);
    const int qrow = 16 * (wave & 3) + i;
    const int b = q0 + qrow;
    const float qn = NEED_NORM ? qn2[qrow] : 0.f;
    const float qsc = mode_is_f16(MODE) ? qsc_s[qrow] : 1.f;  // 2^-e of this lane's query row (LDS header)
    const bool partial_tile = s0 + BS > N;  // only the last support tile has rows past the bank
    const int *win_lo = nullptr, *win_hi = nullptr;
    if constexpr (out_is_win(OUT)) {   // the window's arrays ride in on `scores` / `ws_den`; the tile sums lie behind the maxima
        win_lo = reinterpret_cast<const int*>(scores);
        win_hi = reinterpret_cast<const int*>(ws_den);
        ws_den = ws_m + fused_den_after_m(n_stiles, B);
    }

    float sc[RS][4];
    float mloc = -INFINITY;
    if (consumer) {
        // OUT_WGT: this lane's row weights, requested before the scores are finished.  The addresses of the partial last tile
        // are clamped to the bank (those scores become -inf below whatever is added to them).
        float4 lw[OUT == OUT_WGT ? RS : 1];
        if constexpr (OUT == OUT_WGT) {
#pragma unroll
            for (int r = 0; r < RS; ++r) {
                const int j = s0 + 16 * r + 4 * g;
                if (!partial_tile) lw[r] = *reinterpret_cast<const float4*>(row_logw + j);
                else lw[r] = make_float4(row_logw[min(j, N - 1)], row_logw[min(j + 1, N - 1)], row_logw[min(j + 2, N - 1)],
                                         row_logw[min(j + 3, N - 1)]);
            }
        }
        // per-row score factors (nw_internal.h, ScoreFactors): x = acc * K * Cq + (Base + Bq)
        using SF = ScoreFactors<KIND>;
        float Cq, Bq;
        SF::query(qn, qsc, scale, Cq, Bq);
#pragma unroll
        for (int r = 0; r < RS; ++r) {
            float4 n2 = make_float4(0.f, 0.f, 0.f, 0.f), s4 = make_float4(1.f, 1.f, 1.f, 1.f);
            if (NEED_NORM) n2 = *reinterpret_cast<const float4*>(sn2 + 16 * r + 4 * g);
            if (mode_is_f16(MODE)) s4 = *reinterpret_cast<const float4*>(ssc + 16 * r + 4 * g);  // 2^-e of the support rows
            const float nn[4] = {n2.x, n2.y, n2.z, n2.w}, ss[4] = {s4.x, s4.y, s4.z, s4.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float K, Base;
                SF::support(nn[e], ss[e], K, Base);
                if constexpr (OUT == OUT_CAND_WIN || OUT == OUT_WGT) {
                    // (OUT_WGT: with zero weights the weighted head returns the windowed head's bits, OUT_WIN's, which round
                    // `Base + Bq` like the kernels without a window do; test_head_weighted_gpu.py holds the two to each other
                    // at every tile height.)
                    // The windowed search returns nw_knn_f32's scores bit for bit, and in `Base + Bq` those depend on
                    // how the compiler contracts the sum in the kernels without a window: a fused multiply-add for every
                    // element but the lane's last one of the tile, whose product shares a packed multiply with the
                    // query's and is rounded on its own.  Spelled out here, where another contraction would be another
                    // result (test_knn_window_gpu.py holds the two to each other at every tile height).
                    sc[r][e] = SF::finish(__builtin_fmaf(acc[r][e], K * Cq, SF::base_plus(nn[e], Bq, r == RS - 1 && e == 3)));
                } else {
                    sc[r][e] = SF::finish(__builtin_fmaf(acc[r][e], K * Cq, Base + Bq));
                }
            }
        }
        if constexpr (OUT == OUT_WGT) {
            // score + a in base-2 units, before every mask and the tile maximum: all of them see the weighted score
            // (a = -inf: the row leaves numerator and denominator alike)
#pragma unroll
            for (int r = 0; r < RS; ++r) {
                const float aw[4] = {lw[r].x, lw[r].y, lw[r].z, lw[r].w};
#pragma unroll
                for (int e = 0; e < 4; ++e) sc[r][e] = __builtin_fmaf(aw[e], L2E, sc[r][e]);
            }
        }
        if (partial_tile) {
#pragma unroll
            for (int r = 0; r < RS; ++r)
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (s0 + 16 * r + 4 * g + e >= N) sc[r][e] = -INFINITY;
        }
        if constexpr (OUT == OUT_CAND) {
            tile_candidates<RS>(sc, reinterpret_cast<unsigned*>(scores), ws_lab, B, N, b, s0, g, st, n_stiles, k);
            return;
        }
        if constexpr (OUT == OUT_CAND_WIN) {
            tile_candidates<RS, true>(sc, reinterpret_cast<unsigned*>(scores), ws_lab, B, N, b, s0, g, st, n_stiles, k, ws_nrun,
                                      reinterpret_cast<const int*>(ws_m));
            return;
        }
        if constexpr (OUT == OUT_WIN) window_scores<RS>(sc, win_lo, win_hi, (k & WIN_EXCLUDE) != 0, b, B, N, s0, g);
        if constexpr (OUT == OUT_WGT) {   // (the window is optional beside the weights)
            if (win_lo) window_scores<RS>(sc, win_lo, win_hi, (k & WIN_EXCLUDE) != 0, b, B, N, s0, g);
        }
#pragma unroll
        for (int r = 0; r < RS; ++r) mloc = fmaxf(mloc, fmaxf(fmaxf(sc[r][0], sc[r][1]), fmaxf(sc[r][2], sc[r][3])));
        if (WRITE_SCORES && b < B) {  // natural units for the caller (backward, neighbour search)
            float* orow = scores + (size_t)b * N;
            const bool vec_ok = (N & 3) == 0;
#pragma unroll
            for (int r = 0; r < RS; ++r) {
                const int j = s0 + 16 * r + 4 * g;
                if (j >= N) continue;
                if (vec_ok) {
                    *reinterpret_cast<float4*>(orow + j) =
                        make_float4(sc[r][0] * LN2, sc[r][1] * LN2, sc[r][2] * LN2, sc[r][3] * LN2);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (j + e < N) orow[j + e] = sc[r][e] * LN2;
                }
            }
        }
        // tile-local max over the wave's 16 query columns: lanes i, i+16, i+32, i+48 hold one query
        mloc = group4_max(mloc);
    }
    if constexpr (out_is_cand(OUT)) return;   // (the loader waves)
    NW_FSTAMP(3);

    // ---- 2^(u - mu) and its sums over the runs of equal labels, on the matrix cores:
    //   P[run][query] = sum_t [runid_t == run] * E[t][query]
    // E is already laid out as an MFMA B operand (lane (i,g) holds E[16r+4g+e][query i]: for fixed
    // (r,e) the four lane groups are the four k-slots of one 16x16x4 MFMA), the indicator is the A
    // operand (lane (i,g) supplies [runid[16r+4g+e] == run_base + i]), so 4*RS MFMAs per 16 runs give
    // every lane its four (run, query) sums: no LDS atomics, no divergence, bit-reproducible.
    if (consumer) {
        float dloc = 0.f;
        float msub = mloc;
        if constexpr (out_is_win(OUT)) {
            // dead pairs (mloc = -inf: the window, or the weights, keep no row of the tile for this query).  A wave all of whose
            // sixteen queries are dead stores their zeros and goes; a dead query among live ones takes the sums below with
            // 2^(-inf - 0) = 0 in every element (-inf - -inf would be NaN), which leaves the same zeros.
            const bool dead = mloc == -INFINITY;
            if (__all(dead)) {
                const int nrun = nrun_s[0];
                if (b < B) {
                    for (int run = g; run < nrun; run += 4) ws_num[((size_t)st * BS + run) * B + b] = 0.f;
                    if (g == 0) {
                        ws_m[(size_t)st * B + b] = -INFINITY;
                        ws_den[(size_t)st * B + b] = 0.f;
                    }
                }
                if (qt == 0) {   // this wave's share of the run table (below)
                    if (tid == 0) ws_nrun[st] = nrun;
                    for (int x = tid; x < nrun; x += TILE_THREADS) ws_lab[(size_t)st * BS + x] = runlab[x];
                }
                return;
            }
            msub = dead ? 0.f : mloc;
        }
#pragma unroll
        for (int r = 0; r < RS; ++r)
#pragma unroll
            for (int e = 0; e < 4; ++e) sc[r][e] = __builtin_amdgcn_exp2f(sc[r][e] - msub);  // 2^-inf = 0 for padded rows
        // Run sums.  A run is a RANGE of tile rows: with the first rows b1, b2 of runs 1 and 2 the
        // membership of row t is a clamped difference, [t < b] = clamp(b - t, 0, 1) -- for up to three
        // runs (a class-sorted bank has one or two per tile) 2-7 VALU ops per element instead of a
        // dependent chain of 4*RS fp32 MFMAs; more runs go through the indicator MFMAs.
        const int nrun = nrun_s[0];
        if (nrun <= 3) {
            float S0[2] = {0.f, 0.f}, S1[2] = {0.f, 0.f}, S2[2] = {0.f, 0.f};
            if (nrun == 1) {
#pragma unroll
                for (int r = 0; r < RS; ++r) S0[r & 1] += (sc[r][0] + sc[r][1]) + (sc[r][2] + sc[r][3]);
            } else if (nrun == 2) {
                const float L1 = (float)(nrun_s[1] - 4 * g), M1 = 1.f - L1;
#pragma unroll
                for (int r = 0; r < RS; ++r)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float c = (float)(16 * r + e), ev = sc[r][e];
                        S0[e & 1] = __builtin_fmaf(__builtin_amdgcn_fmed3f(L1 - c, 0.f, 1.f), ev, S0[e & 1]);  // [t <  b1]
                        S1[e & 1] = __builtin_fmaf(__builtin_amdgcn_fmed3f(c + M1, 0.f, 1.f), ev, S1[e & 1]);  // [t >= b1]
                    }
            } else {
                const float L1 = (float)(nrun_s[1] - 4 * g);
                const float M2 = 1.f - (float)(nrun_s[2] - 4 * g);
#pragma unroll
                for (int r = 0; r < RS; ++r)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float c = (float)(16 * r + e), ev = sc[r][e];
                        const float w1 = __builtin_amdgcn_fmed3f(L1 - c, 0.f, 1.f);  // [t <  b1]
                        const float u2 = __builtin_amdgcn_fmed3f(c + M2, 0.f, 1.f);  // [t >= b2]
                        S0[e & 1] = __builtin_fmaf(w1, ev, S0[e & 1]);
                        S2[e & 1] = __builtin_fmaf(u2, ev, S2[e & 1]);
                        S1[e & 1] = __builtin_fmaf((1.f - w1) - u2, ev, S1[e & 1]);  // exact 0 / 1
                    }
            }
            const float s0v = group4_sum(S0[0] + S0[1]);
            float s1v = 0.f, s2v = 0.f;
            if (nrun >= 2) s1v = group4_sum(S1[0] + S1[1]);
            if (nrun == 3) s2v = group4_sum(S2[0] + S2[1]);
            dloc = (s0v + s1v) + s2v;
            if (g == 0 && b < B) {
                ws_num[((size_t)st * BS) * B + b] = s0v;
                if (nrun >= 2) ws_num[((size_t)st * BS + 1) * B + b] = s1v;
                if (nrun == 3) ws_num[((size_t)st * BS + 2) * B + b] = s2v;
            }
        } else {
            float dl[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int r = 0; r < RS; ++r) dl[r & 3] += (sc[r][0] + sc[r][1]) + (sc[r][2] + sc[r][3]);
            dloc = group4_sum((dl[0] + dl[1]) + (dl[2] + dl[3]));
            for (int run_base = 0; run_base < nrun; run_base += 16) {
                // four independent accumulation chains (a dependent fp32 MFMA waits 40 cycles, an independent
                // one issues every 32), added at the end in a fixed order
                f32x4 P0 = {0.f, 0.f, 0.f, 0.f}, P1 = P0, P2 = P0, P3 = P0;
                const int want = run_base + i;
#pragma unroll
                for (int r = 0; r < RS; ++r) {
                    const int4 rid = *reinterpret_cast<const int4*>(runid + 16 * r + 4 * g);
                    P0 = __builtin_amdgcn_mfma_f32_16x16x4f32(rid.x == want ? 1.f : 0.f, sc[r][0], P0, 0, 0, 0);
                    P1 = __builtin_amdgcn_mfma_f32_16x16x4f32(rid.y == want ? 1.f : 0.f, sc[r][1], P1, 0, 0, 0);
                    P2 = __builtin_amdgcn_mfma_f32_16x16x4f32(rid.z == want ? 1.f : 0.f, sc[r][2], P2, 0, 0, 0);
                    P3 = __builtin_amdgcn_mfma_f32_16x16x4f32(rid.w == want ? 1.f : 0.f, sc[r][3], P3, 0, 0, 0);
                }
                const f32x4 P = (P0 + P1) + (P2 + P3);
                // P[j] = sum of run (run_base + 4g + j) for query column i
                if (b < B) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int run = run_base + 4 * g + j;
                        if (run < nrun) ws_num[((size_t)st * BS + run) * B + b] = P[j];
                    }
                }
            }
        }
        NW_FSTAMP(4);
        if (g == 0 && b < B) {
            ws_m[(size_t)st * B + b] = mloc;
            ws_den[(size_t)st * B + b] = dloc;
        }
    }
    NW_FSTAMP(5);
    if (qt == 0) {  // run table is a property of the support tile: written once per tile
        const int nrun = *nrun_s;
        if (tid == 0) ws_nrun[st] = nrun;
        for (int x = tid; x < nrun; x += TILE_THREADS) ws_lab[(size_t)st * BS + x] = runlab[x];
    }
}


// OUT_CAND: sy is not read, `scores` / `ws_lab` are CandOut's key / row arrays and `C` carries k.
// OUT_CAND_WIN: `C` carries CAND_EXCLUDE besides and `ws_nrun` / `ws_m` are the row window's two arrays.
// OUT_WIN: `scores` / `ws_den` are the row window's two arrays, `C` carries WIN_EXCLUDE besides the class count.
// OUT_WGT: as OUT_WIN (both window arrays may be null), and `row_logw` holds the bank rows' log-weights; null otherwise.
template <int RS, int KIND, int OUT, int MODE>
__global__ __launch_bounds__(TILE_THREADS, (RS <= 5 ? 4 : 2)) void nw_fused_kernel(
    const float* __restrict__ q, const float* __restrict__ s, const int64_t* __restrict__ sy,
    const float* __restrict__ s_norm2, const float* __restrict__ s_scale, const float* __restrict__ q_norm2,
    const float* __restrict__ q_scale, const float* __restrict__ logit_scale,
    float* __restrict__ scores, float* __restrict__ ws_m,
    float* __restrict__ ws_den, int* __restrict__ ws_nrun, int* __restrict__ ws_lab,
    float* __restrict__ ws_num, int B, int N, int d, int C, int n_stiles, int n_qtiles,
    const float* __restrict__ row_logw) {
    using Cfg = TileCfg<RS>;
    constexpr int BS = Cfg::BS;
    constexpr bool NEED_NORM = (KIND != NW_SCORE_DOT);
    extern __shared__ __attribute__((aligned(16))) char smem[];
    // header: qn2[64] | qsc[64] | sn2[RUN_CAP] | ssc[RUN_CAP] | runid[RUN_CAP] | runlab[RUN_CAP] | nrun ; then the ring
    float* qn2 = reinterpret_cast<float*>(smem);
    float* qsc_s = qn2 + 64;      // MODE_F16: per-query row scale 2^-e
    float* sn2 = qsc_s + 64;
    float* ssc = sn2 + RUN_CAP;   // MODE_F16: per-support row scale 2^-e
    int* runid = reinterpret_cast<int*>(ssc + RUN_CAP);
    int* runlab = runid + RUN_CAP;
    int* nrun_s = runlab + RUN_CAP;
    constexpr int HDR = (128 + 4 * RUN_CAP + 4) * 4;
    static_assert(HDR % 16 == 0, "stage buffers must stay 16-byte aligned");
    float4* stage = reinterpret_cast<float4*>(smem + HDR);

    int qt, st;
    if (!decode_block(n_stiles, n_qtiles, qt, st)) return;
    const int q0 = qt * BQ, s0 = st * BS;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int i = lane & 15, g = lane >> 4;
    NW_FSTAMP(0);

    // cached support norms: fetched now, long before the epilogue needs them (the DMA loop never
    // touches sn2 in this mode)
    if ((MODE == MODE_DMA_SN || mode_is_f16(MODE)) && NEED_NORM) {
        for (int t = tid; t < BS; t += TILE_THREADS) sn2[t] = s_norm2[min(s0 + t, N - 1)];
    }
    if (mode_is_f16(MODE)) {
        for (int t = tid; t < BS; t += TILE_THREADS) ssc[t] = s_scale[min(s0 + t, N - 1)];
    }
    if (MODE == MODE_F16) {  // MODE_F16Q: the consumer waves fill qn2 / qsc_s themselves
        if (NEED_NORM)
            for (int t = tid; t < BQ; t += TILE_THREADS) qn2[t] = q_norm2[min(q0 + t, B - 1)];
        for (int t = tid; t < BQ; t += TILE_THREADS) qsc_s[t] = q_scale[min(q0 + t, B - 1)];
    }
    // ---- runs of equal consecutive labels inside this support tile (one wave)
    if (!out_is_cand(OUT) && wave == 0) {
        int lab[3];
        load_tile_labels<BS>(sy, s0, N, out_is_win(OUT) ? C & (WIN_EXCLUDE - 1) : C, lane, lab);
        run_scan_wave<BS>(lab, lane, runid, runlab, nrun_s);
    }

    NW_FSTAMP(1);
    // the K walk of every support tile starts at a different chunk (see tile_core.h: spreads the
    // simultaneous requests of all workgroups over the memory channels); the workgroups that share
    // a support tile keep the same order so that they still hit each other's lines in L2
    const int nk = (d + BK - 1) / BK;
    const int rot = st % nk;
    f32x4 acc[RS];
    if (mode_is_f16(MODE)) {
        tile_dots_f16x2<RS, MODE == MODE_F16Q>(q, s, B, N, d, q0, s0, stage, acc, rot, qn2, qsc_s);
        __syncthreads();  // header tables written at kernel start are visible; the ring is dead
    } else if (MODE == MODE_REG) {
        tile_dots<RS, NEED_NORM>(q, s, B, N, d, q0, s0, stage, qn2, sn2, acc, rot);
    } else {
        tile_dots_dma<RS, NEED_NORM, NEED_NORM && MODE == MODE_DMA>(q, s, B, N, d, q0, s0, stage, qn2, sn2, acc, rot);
    }
    // (both end behind a barrier: the run tables above and the norms are visible, and the stage
    //  buffers are dead from here on)
    if (MODE != MODE_DMA_SN && !mode_is_f16(MODE) && NEED_NORM && s_norm2 != nullptr) {  // cached norms win over computed ones
        for (int t = tid; t < BS; t += TILE_THREADS) sn2[t] = s_norm2[min(s0 + t, N - 1)];
        __syncthreads();
    }

    NW_FSTAMP(2);
    fused_epilogue<RS, KIND, OUT, MODE>(acc, qn2, sn2, ssc, runid, runlab, nrun_s, qsc_s, logit_scale,
                                        scores, ws_m, ws_den, ws_nrun, ws_lab, ws_num, B, N, q0, s0, qt, st, n_stiles, C, row_logw);
    NW_FSTAMP(6);
}


constexpr size_t FUSED_HDR = (128 + 4 * RUN_CAP + 4) * 4;

// The queries as the tile kernel reads them: the caller's raw rows (norm2 = scale = nullptr), or their split / packed form.
struct QueryRows {
    const float *rows, *norm2, *scale;
};

template <int RS, int KIND>
int launch_f16p(const FusedArgs& a, const FusedPlan& p, const QueryRows& q, const FusedWs& ws);
template <int KIND, bool HALF, bool CAND>
int launch_p12(const FusedPlan& p, const FusedArgs& a, const QueryRows& q, const FusedWs& ws);

// Executes a plan of plan_fused (fused.hip) on tiles of RS blocks: workspace layout, the optional run-table launch and
// query-split / pack launch (into the query areas of the call's FwdLayout, or into the CandOut), one tile kernel, the
// run merge.  Which of them, and with which grid and LDS, is the plan's business; nothing is decided here.
template <int RS, int KIND>
int launch_fused_rs(const FusedArgs& a, const FusedPlan& p) {
    constexpr int BS = 16 * RS;
    const CandOut* cand = a.cand;
    hipStream_t st = a.st;
    FusedWs ws = {};
    if (!cand) {   // (candidate output: the caller's CandOut is all the kernel writes)
        if (!a.ws || !a.ws->base) return NW_ERR_WORKSPACE;
        const size_t need = fused_layout(a.B, p.n_stiles, BS, a.ws->base + a.ws->main.off, &ws, a.C);
        if (need > a.ws->main.bytes) return NW_ERR_WORKSPACE;
    }
    if (p.status != NW_OK) return p.status;
    if (p.run_tables && !bank_tables_take(a.sy, a.N, a.C, p.n_stiles, BS, &ws)) {  // once per launch (ws.runid / nrun / lab / bnd)
        const int rc = launch_run_tables(ws, a.sy, a.N, a.C, p.n_stiles, BS, st);
        if (rc != NW_OK) return rc;
    }
    QueryRows q = {a.q, nullptr, nullptr};
    if (p.split_queries) {
        float* const qr = cand ? cand->q_rows : a.ws->at(a.ws->q_rows);
        float* const qsc = cand ? cand->q_scale : a.ws->at(a.ws->q_scale);
        float* const qn = cand ? cand->q_norm2 : a.ws->at(a.ws->q_norm2);
        const int rc = p.form == FORM_HALF ? launch_pack_rows_f16(a.q, qr, qsc, qn, a.B, a.d, st) : launch_split_rows(a.q, qr, qsc, qn, a.B, a.d, st);
        if (rc != NW_OK) return rc;
        q = {qr, qn, qsc};
    }
    // OUT_CAND: CandOut's key / row arrays stand where the scores and the run labels go, k where the class count goes
    // (nw_fused_kernel); ws is all null then, and the row window's arrays (read only) stand where the tile maxima and
    // the run counts go.
    // OUT_WIN: the head's row window stands where the scores and the tile sums go, its flag beside the class count; the
    // kernel finds the tile sums behind the tile maxima (fused_den_after_m).
    // OUT_WGT: the same, with the row weights in the kernel's last argument (null for every other output).
    const bool head_window = out_is_win(p.out);
    float* scores = cand ? reinterpret_cast<float*>(cand->key) : head_window ? reinterpret_cast<float*>(const_cast<int*>(a.win_lo)) : a.scores;
    int* lab = cand ? cand->row : ws.lab;
    const bool window = cand && cand->win_lo && cand->win_hi;
    const int c_or_k = cand ? (cand->k | (window && cand->win_exclude ? CAND_EXCLUDE : 0))
                            : (a.C | (head_window && a.win_exclude ? WIN_EXCLUDE : 0));
    if (window) {
        ws.nrun = const_cast<int*>(cand->win_lo);
        ws.m = reinterpret_cast<float*>(const_cast<int*>(cand->win_hi));
    }
#define NW_TILE(OUT_, MODE_)                                                                                           \
    hipLaunchKernelGGL((nw_fused_kernel<RS, KIND, OUT_, MODE_>), dim3(p.grid), dim3(TILE_THREADS), p.lds_bytes, st, q.rows, \
                       a.s, a.sy, a.s_norm2, a.s_scale, q.norm2, q.scale, a.ls, scores, ws.m, ws.den, ws.nrun, lab, ws.num, \
                       a.B, a.N, a.d, c_or_k, p.n_stiles, p.n_qtiles, p.out == OUT_WGT ? a.row_logw : nullptr)
#define NW_TILE_CASE(MODE_) \
    case MODE_: if (p.out == OUT_SCORES) NW_TILE(OUT_SCORES, MODE_); else NW_TILE(OUT_NONE, MODE_); break
    if (p.out == OUT_CAND && p.persistent) {   // half-precision rows: the 256-query kernel's candidate form (nw_knn_f16)
        if constexpr (RS == 8) {
            if (p.form == FORM_HALF && p.variant == 3) return launch_p12<KIND, true, true>(p, a, q, ws);
        }
        return NW_ERR_UNSUPPORTED;
    }
    if (p.out == OUT_CAND) {   // the launch of the score-writing call of this shape (tile height, raw or split queries, grid)
        // (RS = 12 on split operands exists only under the tile_rs knob and spills there: no candidate form of it)
        if constexpr (RS == 12) {
            return NW_ERR_UNSUPPORTED;
        } else {
            if (window) {
                if (p.mode == MODE_F16Q) NW_TILE(OUT_CAND_WIN, MODE_F16Q); else NW_TILE(OUT_CAND_WIN, MODE_F16);
            } else {
                if (p.mode == MODE_F16Q) NW_TILE(OUT_CAND, MODE_F16Q); else NW_TILE(OUT_CAND, MODE_F16);
            }
            NW_CHECK_LAUNCH();
            return NW_OK;
        }
    }
    if (out_is_win(p.out)) {   // the windowed head: the tile kernel of the windowed search at this shape, then the run merge
        if constexpr (RS == 12) {
            return NW_ERR_UNSUPPORTED;
        } else {
            const bool weighted = p.out == OUT_WGT;   // (its window is optional: both arrays or neither)
            if (p.persistent || p.run_tables || !mode_is_f16(p.mode)) return NW_ERR_UNSUPPORTED;
            if (weighted ? (!a.row_logw || !a.win_lo != !a.win_hi) : (!a.win_lo || !a.win_hi)) return NW_ERR_UNSUPPORTED;
            float* const den = ws.den;
            if (den != ws.m + fused_den_after_m(p.n_stiles, a.B) || a.C >= WIN_EXCLUDE) return NW_ERR_UNSUPPORTED;
            ws.den = reinterpret_cast<float*>(const_cast<int*>(a.win_hi));
            if (weighted) {
                if (p.mode == MODE_F16Q) NW_TILE(OUT_WGT, MODE_F16Q); else NW_TILE(OUT_WGT, MODE_F16);
            } else {
                if (p.mode == MODE_F16Q) NW_TILE(OUT_WIN, MODE_F16Q); else NW_TILE(OUT_WIN, MODE_F16);
            }
            ws.den = den;
            NW_CHECK_LAUNCH();
            return launch_merge_runs(ws, a.out, a.lse, a.m, a.den, a.num, a.B, a.C, p.n_stiles, BS, st);
        }
    }
    const int timer_slot = tile_timer_start(st);
    if (p.persistent) {
        const int rc = launch_f16p<RS, KIND>(a, p, q, ws);
        if (rc != NW_OK) return rc;
    } else {
        switch (p.mode) {
            NW_TILE_CASE(MODE_REG);
            NW_TILE_CASE(MODE_DMA);
            NW_TILE_CASE(MODE_DMA_SN);
            NW_TILE_CASE(MODE_F16);
            NW_TILE_CASE(MODE_F16Q);
        }
    }
#undef NW_TILE_CASE
#undef NW_TILE
    tile_timer_stop(timer_slot, st);
    NW_CHECK_LAUNCH();
    return launch_merge_runs(ws, a.out, a.lse, a.m, a.den, a.num, a.B, a.C, p.n_stiles, BS, st);
}

}  // namespace

// Every form goes through here: the half-precision one (FORM_HALF) is a plan on tiles of 128 supports like any other.
template <int KIND>
int launch_fused_kind(const FusedArgs& a, const FusedPlan& p) {
    switch (p.rs) {
        case 2: return launch_fused_rs<2, KIND>(a, p);
        case 4: return launch_fused_rs<4, KIND>(a, p);
        case 5: return launch_fused_rs<5, KIND>(a, p);
        case 6: return launch_fused_rs<6, KIND>(a, p);
        case 8: return launch_fused_rs<8, KIND>(a, p);
        case 10: return launch_fused_rs<10, KIND>(a, p);
        default: return launch_fused_rs<12, KIND>(a, p);
    }
}

}  // namespace nw
#include "fused_f16p.h"
#include "fused_f16p12.h"
namespace nw {
namespace {
// The one launch of nw_fused_f16p_kernel_w12 (256-query tiles of 128 supports, fused_f16p12.h).  HALF: half-precision rows
// (a.s / s_scale / s_norm2 from nw_pack_rows_f16, the queries packed likewise); their stride in floats is d / 2 -- the
// loader and the stage count follow from it.  CAND: the candidate output (a.cand's key / row arrays where the tile
// maxima / sums go, no run tables, no partials: ws is all null).
template <int KIND, bool HALF, bool CAND>
int launch_p12(const FusedPlan& p, const FusedArgs& a, const QueryRows& q, const FusedWs& ws) {
    static const bool attr = hipFuncSetAttribute(reinterpret_cast<const void*>(nw_fused_f16p_kernel_w12<KIND, HALF, CAND>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)P12::LDS_BYTES) == hipSuccess;
    (void)attr;
    float* m = CAND ? reinterpret_cast<float*>(a.cand->key) : ws.m;
    float* den = CAND ? reinterpret_cast<float*>(a.cand->row) : ws.den;
    hipLaunchKernelGGL((nw_fused_f16p_kernel_w12<KIND, HALF, CAND>), dim3(p.workgroups), dim3(P12::THREADS), p.lds_bytes, a.st,
                       q.rows, a.s, a.s_norm2, a.s_scale, q.norm2, q.scale, a.ls, ws.runid, ws.nrun, ws.bnd, m, den, ws.num, a.B,
                       a.N, HALF ? a.d / 2 : a.d, p.n_stiles, (a.B + P12::BQP - 1) / P12::BQP, p.qgroup, CAND ? a.cand->k : 0);
    NW_CHECK_LAUNCH();
    return NW_OK;
}

// The persistent kernel of the plan's variant (and, for variant 3, form); the run tables are the caller's job.  The
// persistent kernels exist for tiles of 128 supports only: plan_fused gives no other height a persistent plan.
template <int RS, int KIND>
int launch_f16p(const FusedArgs& a, const FusedPlan& p, const QueryRows& q, const FusedWs& ws) {
    if constexpr (RS == 8) {
#define NW_LAUNCH_P(TWO_, QB_)                                                                                        \
    hipLaunchKernelGGL((nw_fused_f16p_kernel<RS, KIND, TWO_, QB_>), dim3(p.workgroups), dim3(TILE_THREADS), p.lds_bytes, \
                       a.st, q.rows, a.s, a.s_norm2, a.s_scale, q.norm2, q.scale, a.ls, ws.runid, ws.nrun, ws.bnd, ws.m, \
                       ws.den, ws.num, a.B, a.N, a.d, p.n_stiles, (a.B + 64 * (QB_) - 1) / (64 * (QB_)), p.qgroup)
        switch (p.variant) {
            case 3: return p.form == FORM_HALF ? launch_p12<KIND, true, false>(p, a, q, ws) : launch_p12<KIND, false, false>(p, a, q, ws);
            case 2: NW_LAUNCH_P(false, 2); break;
            case 1: NW_LAUNCH_P(true, 1); break;
            default: NW_LAUNCH_P(false, 1); break;
        }
#undef NW_LAUNCH_P
        NW_CHECK_LAUNCH();
        return NW_OK;
    } else {
        return NW_ERR_UNSUPPORTED;
    }
}
}  // namespace

#define NW_INSTANTIATE_FUSED_KIND(K) template int launch_fused_kind<K>(const FusedArgs&, const FusedPlan&);

}  // namespace nw
