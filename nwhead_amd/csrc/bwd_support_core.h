// bwd_support_core.h -- the skeleton the three SUPPORT-SIDE gradient kernels over a resident split bank share:
// bwd_values_support.hip (the value head: gradients to the values and the row weights), bwd_support.hip (the class
// head: gradient to the bank rows) and bwd_values_bank.hip (the value head: gradient to the bank rows).  All contract, over the QUERIES, a (B, N) matrix X that is recomputed tile by tile with
// an operand of width `width` (gout, T columns; q, d columns): a workgroup owns one 64-row support tile, a slab of 32 * NCH
// operand columns and a contiguous chunk of the 64-query tiles.  What is the same in both is here once: the plan, the
// operand's one exponent and its pack in MFMA lane order, the consumer lane's window rule and weight W, the h + l write of
// X to LDS, tile += X^T operand on v_mfma_f32_16x16x32_f16 in the order lh + hl + hh, the exchange of the per-row sums at
// the end, and the launch of the main kernel.  Each file keeps its numerics (its header comment), its prologue, its own
// workspace areas and what turns W into X.  The two gradients to the BANK ROWS (operand q, X the signed coefficient A) share
// more, at the end of the file: the workspace areas behind their own, the workgroup's running exponent, the store of the
// still-scaled tile and the finish kernel.  Every device piece is __forceinline__: the kernels' code is what it was with the
// pieces written out (the Makefile's resource rules hold for every unit).
#pragma once
#include "nw_internal.h"
#include "tile_dma.h"
#include "tile_f16.h"

namespace nw {
namespace {

constexpr int SRS = 4;            // support blocks per tile
constexpr int SBS = 16 * SRS;     // 64 bank rows per tile
constexpr int X_STRIDE = BQ + 8;  // halves per row of the exchanged X: 144 bytes (conflict-free for the 2-byte writes)
static_assert((size_t)2 * SBS * X_STRIDE * 2 <= DmaCfg<SRS>::STAGE_BYTES, "X halves inside the ring");
static_assert((size_t)BQ * SBS * 4 <= DmaCfg<SRS>::STAGE_BYTES, "the row-sum exchange inside the ring");
constexpr int S_CUS = 256;        // workgroups that fill the chip
constexpr float HALF_MAX = 60000.f;
constexpr int S_NCH_MAX = 8, S_NCH_MIN = 4;   // the slab widths that are shipped (Makefile: no scratch in either)

struct SupPlan {
    int n_stiles, n_qtiles, nch, nslabs, nchunks, tpc;
};

// Slab width: the narrow one when it takes all of the operand's width.  Query chunks: one when the support tiles and slabs
// alone fill the chip, otherwise as many as do (at most the query tiles); a positive query_chunks is taken, clamped to the
// query tiles.
inline SupPlan sup_plan(int64_t B, int64_t N, int64_t width, int query_chunks) {
    const int64_t n_stiles = (N + SBS - 1) / SBS, n_qtiles = (B + BQ - 1) / BQ, nk = width / BK;
    const int nch = nk <= S_NCH_MIN ? S_NCH_MIN : S_NCH_MAX;
    const int64_t nslabs = (nk + nch - 1) / nch;
    int64_t want;
    if (query_chunks > 0) {
        want = query_chunks;
    } else {
        const int64_t wgs = n_stiles * nslabs;
        want = wgs >= S_CUS ? 1 : (S_CUS + wgs - 1) / wgs;
    }
    if (want > n_qtiles) want = n_qtiles;
    if (want < 1) want = 1;
    const int64_t tpc = (n_qtiles + want - 1) / want, nchunks = (n_qtiles + tpc - 1) / tpc;
    return {(int)n_stiles, (int)n_qtiles, nch, (int)nslabs, (int)nchunks, (int)tpc};
}

// The areas of a workspace, each a multiple of 256 bytes, in the order they are taken; base == nullptr: the sizes alone.
struct SupCarve {
    char* base;
    size_t off = 0;
    template <typename T>
    T* take(size_t bytes) {
        char* ptr = base ? base + off : nullptr;
        off += align256(bytes);
        return reinterpret_cast<T*>(ptr);
    }
};

// the one exponent of the operand: split_exponent of the largest magnitude (0 for an all-zero operand)
__global__ __launch_bounds__(256) void nw_bwd_support_exp_kernel(const float* __restrict__ xmax, int* __restrict__ xexp,
                                                                  int64_t B) {
    __shared__ float red[8];
    float mx = 0.f;
    for (int64_t b = threadIdx.x; b < B; b += 256) mx = fmaxf(mx, xmax[b]);
    mx = block_max(mx, red);
    if (threadIdx.x == 0) *xexp = split_exponent(mx);
}

// x 2^E -> fp16 halves in the B-operand order of the main kernel: thread (query tile, column block, step, lane (i, g))
// packs queries 32 step + 8g .. + 7 of column 16 block + i.  A query past B is a zero.
__global__ __launch_bounds__(256) void nw_bwd_support_pack_kernel(const float* __restrict__ x, const int* __restrict__ xexp,
                                                                   half8* __restrict__ xpack, int64_t B, int64_t width,
                                                                   int64_t total) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int lane = (int)(idx & 63), i = lane & 15, g = lane >> 4;
    const int ks = (int)((idx >> 6) & 1);
    const int64_t ncb = width / 16, blk = idx >> 7;
    const int64_t cb = blk % ncb, qt = blk / ncb;
    const float up = __builtin_ldexpf(1.f, *xexp);
    half8 h, l;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int64_t b = qt * BQ + 32 * ks + 8 * g + k;
        float v = b < B ? x[b * width + 16 * cb + i] * up : 0.f;
        v = __builtin_amdgcn_fmed3f(v, -HALF_MAX, HALF_MAX);   // (only a non-finite input gets here)
        h[k] = (_Float16)v;
        l[k] = (_Float16)(v - (float)h[k]);
    }
    half8* dst = xpack + ((blk * 2 + ks) * 2) * 64 + lane;
    dst[0] = h;
    dst[64] = l;
}

// threads of the pack kernel: [query tile][16-column block][32-query step][h, l][lane], 8 halves each
inline int64_t sup_pack_threads(const SupPlan& p, int64_t width) { return (int64_t)p.n_qtiles * (width / 16) * 128; }

// xmax (B,), from the file's prologue -> the exponent and the packed operand
inline void launch_sup_pack(const float* x, const float* xmax, int* xexp, half8* xpack, int64_t B, int64_t width,
                            const SupPlan& p, hipStream_t st) {
    const int64_t npack = sup_pack_threads(p, width);
    hipLaunchKernelGGL(nw_bwd_support_exp_kernel, dim3(1), dim3(256), 0, st, xmax, xexp, B);
    hipLaunchKernelGGL(nw_bwd_support_pack_kernel, dim3((unsigned)((npack + 255) / 256)), dim3(256), 0, st, x, xexp, xpack, B,
                       width, npack);
}

// A consumer lane's query against the workgroup's support tile [s0, tile_end): query q0 + qrow on the lane, rows
// s0 + 16r + 4g + e in the registers.
struct SupQuery {
    int b, bb;           // the query, and the same clamped to B - 1 for addresses
    float lsev, Cq, Bq;  // lse in base-2 units (+inf: W = 0 in every row), the query's score factors
    unsigned width;      // of the window
    int rel, row0;       // s0 + 4g - lo, s0 + 4g
    bool windowed, exclude, check;
};

// `qn`: |q|^2 (0 for the dot product); `scale`: the clip scale (1 elsewhere), as the caller has it.
template <int KIND>
__device__ __forceinline__ SupQuery sup_query(const float* __restrict__ lse_p, const int* __restrict__ win_lo,
                                              const int* __restrict__ win_hi, bool exclude, int B, int N, int q0, int qrow,
                                              int g, int s0, int tile_end, float qn, float qsc, float scale) {
    constexpr float L2E = 1.44269504088896340736f;
    SupQuery Q;
    Q.b = q0 + qrow, Q.bb = Q.b < B ? Q.b : B - 1;
    const float lse = lse_p[Q.bb];
    // a dead query and a lane past B: W = 2^(u - inf) = 0 in every row
    Q.lsev = (lse == -INFINITY || Q.b >= B) ? INFINITY : lse * L2E;
    Q.windowed = win_lo != nullptr, Q.exclude = exclude;
    int lo = 0, hi = N;
    if (Q.windowed) lo = min(max(win_lo[Q.bb], 0), N), hi = min(max(win_hi[Q.bb], 0), N);   // never used as addresses
    Q.width = hi > lo ? (unsigned)(hi - lo) : 0u;
    ScoreFactors<KIND>::query(qn, qsc, scale, Q.Cq, Q.Bq);
    // the window's rule of the forward (fused_impl.h, OUT_WIN): a pair the window leaves whole skips the comparisons
    const bool whole =
        !Q.windowed || (exclude ? (Q.width == 0u || hi <= s0 || lo >= tile_end) : (lo <= s0 && hi >= tile_end));
    Q.check = !whole || tile_end < s0 + SBS || Q.b >= B;
    Q.rel = s0 + 4 * g - lo, Q.row0 = s0 + 4 * g;
    return Q;
}

// W of the pair (query of the lane, row row0 + t, t = 16r + e) from the tile's dot product: the forward's fused multiply-add
// with the row's log-weight `aw`, 0 where the window, N or B leaves the pair out.  `u`: the raw score in base-2 units.
template <int KIND>
__device__ __forceinline__ float sup_weight(const SupQuery& Q, float dot, float nn, float ss, float aw, int t, int B, int N,
                                            float& u) {
    constexpr float L2E = 1.44269504088896340736f;
    using SF = ScoreFactors<KIND>;
    float K, Base;
    SF::support(nn, ss, K, Base);
    // Base + Bq as ONE fused multiply-add, spelled out (base_plus): that is what the compiler's contraction made of it in both
    // kernels, and left to itself it rounds the product of one pair on its own when it packs it with another multiplication
    u = SF::finish(__builtin_fmaf(dot, K * Q.Cq, SF::base_plus(nn, Q.Bq, false)));   // base-2 units, as the forward
    float W = __builtin_amdgcn_exp2f(__builtin_fmaf(aw, L2E, u) - Q.lsev);
    if (Q.check) {
        bool keep = Q.row0 + t < N && Q.b < B;
        if (Q.windowed) keep = keep && (((unsigned)(Q.rel + t) < Q.width) != Q.exclude);
        W = keep ? W : 0.f;
    }
    return W;
}

// v up = h + l, clamped to [floor, HALF_MAX] (only a non-finite input gets there), to LDS as [row][query]
__device__ __forceinline__ void sup_put_halves(_Float16* Xh, _Float16* Xl, int row, int qrow, float v, float up, float floor) {
    const float x = __builtin_amdgcn_fmed3f(v * up, floor, HALF_MAX);
    const _Float16 h = (_Float16)x;
    Xh[row * X_STRIDE + qrow] = h;
    Xl[row * X_STRIDE + qrow] = (_Float16)(x - (float)h);
}

// All eight waves: tile += X^T operand, K = the 64 queries of tile `qt`.  Wave (rb, hf) owns rows 16 rb .. + 15 and the
// slab's 32-column chunks c = hf, hf + 2, ... below nc.  The A operand is a plain 16-byte LDS read (8 consecutive queries of
// a row); the B operand comes from the packed global buffer, one contiguous 1 KB line per load of a wave.
template <int NCC>
__device__ __forceinline__ void sup_mfma_tile(f32x4 (&gacc)[NCC][2], const _Float16* Xh, const _Float16* Xl,
                                              const half8* __restrict__ xpack, int qt, int ncb, int kc0, int nc, int rb,
                                              int hf, int lane) {
    const int i = lane & 15, g = lane >> 4;
    half8 Ah[2], Al[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
        Ah[ks] = *reinterpret_cast<const half8*>(Xh + (16 * rb + i) * X_STRIDE + 32 * ks + 8 * g);
        Al[ks] = *reinterpret_cast<const half8*>(Xl + (16 * rb + i) * X_STRIDE + 32 * ks + 8 * g);
    }
    auto mm = [](const half8& x, const half8& y, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(x, y, c, 0, 0, 0); };
    const half8* xp = xpack + (size_t)qt * ncb * 256 + lane;
#pragma unroll
    for (int cc = 0; cc < NCC; ++cc) {
        const int c = 2 * cc + hf;
        if (c < nc) {
            half8 Xf[2][2][2];   // [column block][step][h, l]
#pragma unroll
            for (int nb = 0; nb < 2; ++nb)
#pragma unroll
                for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                    for (int hl = 0; hl < 2; ++hl)
                        Xf[nb][ks][hl] = xp[((size_t)(2 * (kc0 + c) + nb) * 2 + ks) * 128 + hl * 64];
            // small terms first, the dominant h*h product last; the two column blocks alternate
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                gacc[cc][0] = mm(Al[ks], Xf[0][ks][0], gacc[cc][0]);
                gacc[cc][1] = mm(Al[ks], Xf[1][ks][0], gacc[cc][1]);
                gacc[cc][0] = mm(Ah[ks], Xf[0][ks][1], gacc[cc][0]);
                gacc[cc][1] = mm(Ah[ks], Xf[1][ks][1], gacc[cc][1]);
                gacc[cc][0] = mm(Ah[ks], Xf[0][ks][0], gacc[cc][0]);
                gacc[cc][1] = mm(Ah[ks], Xf[1][ks][0], gacc[cc][1]);
            }
        }
    }
}

// The consumers' per-lane row sums pm[r][e] (row 16r + 4g + e, the lane's query) -> dst[row], the tile's 64 query slots
// added in order.  The whole workgroup calls it, after the last tile (pmx lies over the ring).
__device__ __forceinline__ void sup_row_sums(const float (&pm)[SRS][4], float* pmx, float* __restrict__ dst, int tid, int wave) {
    const int lane = tid & 63, i = lane & 15, g = lane >> 4;
    if (wave < NCONS) {
#pragma unroll
        for (int r = 0; r < SRS; ++r)
#pragma unroll
            for (int e = 0; e < 4; ++e) pmx[(16 * wave + i) * SBS + 16 * r + 4 * g + e] = pm[r][e];
    }
    __syncthreads();
    if (tid < SBS) {
        float v = 0.f;
        for (int k = 0; k < BQ; ++k) v += pmx[k * SBS + tid];
        dst[tid] = v;
    }
}

// One launch of a main kernel, its dynamic LDS allowed once per process.
template <auto KERNEL, typename Args>
int launch_sup_kernel(const Args& a, size_t lds, unsigned grid, hipStream_t st) {
    static const bool attr =
        hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) == hipSuccess;
    if (!attr) return NW_ERR_LAUNCH;
    hipLaunchKernelGGL(KERNEL, dim3(grid), dim3(TILE_THREADS), lds, st, a);
    return NW_OK;
}
// ... of a score kind at the plan's slab width: KERNEL_MAX / KERNEL_MIN are its instantiations at S_NCH_MAX / S_NCH_MIN
template <auto KERNEL_MAX, auto KERNEL_MIN, typename Args>
int launch_sup_kind(const Args& a, size_t lds, int nch, unsigned grid, hipStream_t st) {
    if (nch == S_NCH_MAX) return launch_sup_kernel<KERNEL_MAX>(a, lds, grid, st);
    return launch_sup_kernel<KERNEL_MIN>(a, lds, grid, st);
}

// ---- what the gradients to the BANK ROWS share beyond the skeleton (bwd_support.hip, bwd_values_bank.hip):
//      gs_j = sum_b A_bj q_b + 2 (sum_b r_bj) s_j with A signed and unbounded, scaled by the workgroup's running exponent.

// The workspace areas of both, behind the file's own (its prologue's results): qmax | qexp | qpack | rp | esc | part
struct SupRowsWs {
    float* qmax;       // [query]: max_k |q_bk|
    int* qexp;
    half8* qpack;      // [query tile][16-column block][32-query step][h, l][lane]: 8 halves each
    float* rp;         // [chunk][row]: rows padded to the tile
    int* esc;          // [chunk][support tile]: the exponent that unscales the chunk's tile
    float* part;       // [chunk][N][d], only with more than one chunk
};
inline void sup_rows_layout(SupCarve& c, int64_t B, int64_t N, int64_t d, const SupPlan& p, SupRowsWs& w) {
    const size_t npad = (size_t)p.n_stiles * SBS;
    w.qmax = c.take<float>((size_t)B * 4);
    w.qexp = c.take<int>(4);
    w.qpack = c.take<half8>((size_t)p.n_qtiles * BQ * d * 4);
    w.rp = c.take<float>((size_t)p.nchunks * npad * 4);
    w.esc = c.take<int>((size_t)p.nchunks * p.n_stiles * 4);
    w.part = c.take<float>(p.nchunks > 1 ? (size_t)p.nchunks * N * d * 4 : 0);
}

// The workgroup's exponent, from the consumer waves' largest |A| of the query tile (wmx[NCONS], behind a barrier): raised
// (a smaller E) when this query tile holds a larger coefficient than any before.  Returns the power of two every accumulator
// of the workgroup is multiplied with before the tile is added (1: none).  Uniform over the workgroup.
__device__ __forceinline__ float sup_running_exponent(const float* wmx, int& Erun, bool& have) {
    static_assert(NCONS == 4, "the four maxima are read as one float4");
    float factor = 1.f;
    const float4 m4 = *reinterpret_cast<const float4*>(wmx);
    const float tmax = fmaxf(fmaxf(m4.x, m4.y), fmaxf(m4.z, m4.w));
    if (tmax > 0.f && tmax < INFINITY) {
        const int En = split_exponent(tmax);
        if (!have || En < Erun) {
            if (have) factor = __builtin_ldexpf(1.f, En - Erun);   // (before: the accumulators are all zero)
            Erun = En;
            have = true;
        }
    }
    return factor;
}

// The chunk's tile, still scaled: gacc[cc][nb][e] of lane (i, g) = gs'[row 16 rb + 4g + e][column 32 (kc0 + 2 cc + hf) + 16 nb + i]
// -> dst (N, d), the chunk's own.
template <int NCC>
__device__ __forceinline__ void sup_rows_store(const f32x4 (&gacc)[NCC][2], float* __restrict__ dst, int N, int d, int s0,
                                               int kc0, int nc, int rb, int hf, int lane) {
    const int i = lane & 15, g = lane >> 4;
#pragma unroll
    for (int cc = 0; cc < NCC; ++cc) {
        const int c = 2 * cc + hf;
        if (c < nc) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int row = s0 + 16 * rb + 4 * g + e;
                if (row < N) {
                    float* at = dst + (size_t)row * d + (size_t)(kc0 + c) * BK + i;
                    at[0] = gacc[cc][0][e];
                    at[16] = gacc[cc][1][e];
                }
            }
        }
    }
}

// gs[j,k] = sum_chunks part[c][j,k] 2^esc[c][tile of j] + 2 (sum_chunks rp[c][j]) s[j,k], chunks in ascending order from +0
// (k in float4s).  With one chunk `part` is gs itself: a thread reads and writes its own four floats.
__global__ __launch_bounds__(256) void nw_bwd_support_rows_finish_kernel(const float* part, const int* __restrict__ esc,
                                                                          const float* __restrict__ rp, const float* __restrict__ s,
                                                                          float* gs, int nchunks, int n_stiles, int64_t N, int64_t d) {
    const int64_t total4 = N * d / 4;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total4) return;
    const int64_t j = (idx * 4) / d, npad = (int64_t)n_stiles * SBS;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    float r = 0.f;
    for (int c = 0; c < nchunks; ++c) {
        const float4 w = *reinterpret_cast<const float4*>(part + ((int64_t)c * total4 + idx) * 4);
        const int e = esc[(int64_t)c * n_stiles + j / SBS];   // a power of two: exact
        v.x += __builtin_ldexpf(w.x, e); v.y += __builtin_ldexpf(w.y, e);
        v.z += __builtin_ldexpf(w.z, e); v.w += __builtin_ldexpf(w.w, e);
        r += rp[(int64_t)c * npad + j];
    }
    const float r2 = 2.f * r;
    const float4 x = *reinterpret_cast<const float4*>(s + idx * 4);
    v.x = __builtin_fmaf(r2, x.x, v.x); v.y = __builtin_fmaf(r2, x.y, v.y);
    v.z = __builtin_fmaf(r2, x.z, v.z); v.w = __builtin_fmaf(r2, x.w, v.w);
    *reinterpret_cast<float4*>(gs + idx * 4) = v;
}

// whether the grids of a call fit: the main kernel's, the pack's, the finish's
inline bool sup_rows_grids_ok(const SupPlan& p, int64_t N, int64_t d) {
    const int64_t wgs = (int64_t)p.n_stiles * p.nslabs * p.nchunks;
    return wgs <= 0x7fffffffLL && (sup_pack_threads(p, d) + 255) / 256 <= 0x7fffffffLL && (N * d / 4 + 255) / 256 <= 0x7fffffffLL;
}
inline void launch_sup_rows_finish(const float* part, const SupRowsWs& w, const float* s, float* gs, const SupPlan& p, int64_t N,
                                   int64_t d, hipStream_t st) {
    const int64_t total4 = N * d / 4;
    hipLaunchKernelGGL(nw_bwd_support_rows_finish_kernel, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, st, part, w.esc,
                       w.rp, s, gs, p.nchunks, p.n_stiles, N, d);
}

}  // namespace
}  // namespace nw
