// bwd_values_support.hip -- gradients of the VALUE head w.r.t. the VALUES and the ROW WEIGHTS over a resident split bank,
// without a (B,N) matrix (gfx950 / MI355X only; nw_bwd_values_support_f32).
//
// The forward (fwd_values.hip) is out_b = sum_j W_bj v_j, W_bj = exp(score_bj + a_j - lse_b) on the rows the window admits
// and 0 elsewhere.  With g the (B,T) upstream gradient:
//     gV_j = sum_b W_bj g_b                              (N,T): d loss / d values
//     ga_j = sum_b W_bj (g_b . v_j - m_b)                (N,):  d loss / d row_logw,   m_b = g_b . out_b
//          = gV_j . v_j - sum_b W_bj m_b
// Both are contractions over the QUERIES of the weight matrix bwd_values.hip recomputes tile by tile, so its skeleton is
// turned around: a workgroup owns one 64-row support tile, a slab of 32 * NCH value columns and a contiguous chunk of the
// 64-query tiles, and loops over the query tiles.  Per query tile it
//   1. recomputes the tile's dot products exactly as bwd_values.hip step 1 does (tile_dots_f16x2<4, true> over q, the split
//      bank rows, d), the forward's window rule, the fused multiply-add for the weight, the dead-query rule; a lane past B
//      holds W = 0;
//   2. the consumer waves hold W "query on the lane, rows 16r + 4g + e in the registers".  They add W m_b to 16 per-lane
//      fp32 sums (the second term of ga: no exchange before the end of the kernel), split W 2^15 into fp16 halves h + l and
//      write both to LDS as [row][query] (the ring is dead by then; 144-byte rows: conflict-free for the 2-byte writes);
//   3. all EIGHT waves then run gV_tile += W^T G on v_mfma_f32_16x16x32_f16, K = the query, in the order lh + hl + hh: wave
//      (rb, hf) owns rows 16 rb .. + 15 and the slab's 32-column chunks c = hf, hf + 2, ...: 32 accumulators at
//      NCH = 8.  The A operand is a plain 16-byte LDS read (8 consecutive queries of a row).  The B operand comes straight
//      from global memory: a prologue packs gout once, split and in MFMA lane order, so that a wave's load is one contiguous
//      1 KB line (B x T x 4 bytes in all; L2-resident, every support tile reads the same lines).
// Scales.  W <= 1, so the fixed scale 2^15 replaces the running row exponent of the sibling kernels: W 2^15 = h + l with an
// absolute error of W of about max(2^-22 W, 2^-40).  The per-query exponents of gout cannot be factored out of a sum over
// queries, so gout is split against ONE exponent, that of max |gout| (a maximum: the same whatever the order): an element's
// absolute error is 2^-22 of itself or 2^-39 of the largest, whichever is larger.  Products are exact, sums are fp32:
//     |error of gV_jt| <~ (2^-21 + B 2^-24) sum_b W_bj |g_bt| + 2^-38 max|g| sum_b W_bj
// Scaling gout by 2^k moves the exponent by k and nothing else: gvalues scales exactly.
// ga: the finished (unscaled) gV tile is multiplied with the fp32 value rows, a lane adding its columns in ascending order,
// the 16 lanes of a row in a fixed exchange tree; the partial sums (wave halves, slabs, query chunks) and the W m sums are
// added by a finish kernel in ascending order, starting from +0.  With gvalues == NULL nothing of size N x T is stored.
// Exact zeros: a row at a = -inf, a row no query's window admits, a dead query (lse = -inf), a row past N and a lane past B
// have W = +0 in both halves; +0 + (+-0) = +0 in every accumulator, so such rows get +0.0 in every column and in glogw.
// A zero column of gout gives a zero column of gvalues.  The value rows enter ga only, and must be finite there.
// Query chunks fill the chip when there are few support tiles; each writes partial tiles, a finish kernel adds them in
// chunk order: no float atomics, two calls give the same bits.
#include "nw_internal.h"
#include "tile_dma.h"
#include "tile_f16.h"

namespace nw {
namespace {

constexpr int SRS = 4;            // support blocks per tile
constexpr int SBS = 16 * SRS;     // 64 bank rows per tile
// qn2[BQ] | qsc[BQ] | sn2[SBS] | ssc[SBS] | law[SBS]
constexpr int S_HDR = (2 * BQ + 3 * SBS) * 4;
static_assert(S_HDR % 16 == 0, "stage buffers must stay 16-byte aligned");
constexpr size_t S_LDS = S_HDR + DmaCfg<SRS>::STAGE_BYTES;
static_assert(S_LDS <= 80 * 1024, "header + ring exceed the LDS of two workgroups per CU");
constexpr int W_STRIDE = BQ + 8;  // halves per row of the exchanged W: 144 bytes
static_assert((size_t)2 * SBS * W_STRIDE * 2 <= DmaCfg<SRS>::STAGE_BYTES, "W halves inside the ring");
static_assert((size_t)BQ * SBS * 4 <= DmaCfg<SRS>::STAGE_BYTES, "the W m exchange inside the ring");
constexpr int S_CUS = 256;        // workgroups that fill the chip
constexpr float HALF_MAX = 60000.f;
constexpr int W_SHIFT = 15;       // W 2^15 <= 32768: inside fp16
constexpr int S_NCH_MAX = 8, S_NCH_MIN = 4;   // the slab widths that are shipped (Makefile: no scratch in either)

struct SupWs {
    float *mb, *gmax;
    int* gexp;
    half8* gpack;      // [query tile][16-column block][32-query step][h, l][lane]: 8 halves each
    float *glp, *pmp;  // [chunk][slab, wave half][row], [chunk][row]: rows padded to the tile
    float* part;       // [chunk][N][T], only with gvalues and more than one chunk
};
struct SupPlan {
    int n_stiles, n_qtiles, nch, nslabs, nchunks, tpc;
};
struct SupArgs {
    const float *q, *s, *s_scale, *s_norm2, *v_rows;
    const int *win_lo, *win_hi;
    const float *lse, *logit_scale, *row_logw;
    float* gv_out;     // gvalues, or the partial tiles, or null
    SupWs ws;
    int want_glogw, exclude, B, N, d, T, n_stiles, n_qtiles, nslabs, nchunks, tpc;
};

// m_b = g_b . out_b and max_t |g_bt|: one workgroup per query.  (A thread adds its columns in order, the block in a fixed
// tree: deterministic.  bwd_values.hip's prologue, which that file keeps to itself, with the maximum beside it.)
__global__ __launch_bounds__(256) void nw_bwd_values_support_prologue_kernel(const float* __restrict__ out,
                                                                              const float* __restrict__ gout,
                                                                              float* __restrict__ mb, float* __restrict__ gmax,
                                                                              int64_t T) {
    __shared__ float red[8];
    const int64_t b = blockIdx.x;
    float t = 0.f, mx = 0.f;
    for (int64_t c = threadIdx.x; c < T; c += 256) {
        const float gv = gout[b * T + c];
        t = __builtin_fmaf(gv, out[b * T + c], t);
        mx = fmaxf(mx, fabsf(gv));
    }
    t = block_sum(t, red);
    mx = block_max(mx, red);
    if (threadIdx.x == 0) mb[b] = t, gmax[b] = mx;
}

// the one exponent of gout: split_exponent of the largest magnitude
__global__ __launch_bounds__(256) void nw_bwd_values_support_gexp_kernel(const float* __restrict__ gmax, int* __restrict__ gexp,
                                                                          int64_t B) {
    __shared__ float red[8];
    float mx = 0.f;
    for (int64_t b = threadIdx.x; b < B; b += 256) mx = fmaxf(mx, gmax[b]);
    mx = block_max(mx, red);
    if (threadIdx.x == 0) *gexp = split_exponent(mx);
}

// gout 2^E -> fp16 halves in the B-operand order of the main kernel: thread (query tile, column block, step, lane (i, g))
// packs queries 32 step + 8g .. + 7 of column 16 block + i.  A query past B is a zero.
__global__ __launch_bounds__(256) void nw_bwd_values_support_pack_kernel(const float* __restrict__ gout, const int* __restrict__ gexp,
                                                                          half8* __restrict__ gpack, int64_t B, int64_t T,
                                                                          int64_t total) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int lane = (int)(idx & 63), i = lane & 15, g = lane >> 4;
    const int ks = (int)((idx >> 6) & 1);
    const int64_t ncb = T / 16, blk = idx >> 7;
    const int64_t cb = blk % ncb, qt = blk / ncb;
    const float up = __builtin_ldexpf(1.f, *gexp);
    half8 h, l;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int64_t b = qt * BQ + 32 * ks + 8 * g + k;
        float x = b < B ? gout[b * T + 16 * cb + i] * up : 0.f;
        x = __builtin_amdgcn_fmed3f(x, -HALF_MAX, HALF_MAX);   // (only a non-finite input gets here)
        h[k] = (_Float16)x;
        l[k] = (_Float16)(x - (float)h[k]);
    }
    half8* dst = gpack + ((blk * 2 + ks) * 2) * 64 + lane;
    dst[0] = h;
    dst[64] = l;
}

template <int KIND, int NCH>
__global__ __launch_bounds__(TILE_THREADS, 2) void nw_bwd_values_support_kernel(const SupArgs a) {
    constexpr bool NEED_NORM = (KIND != NW_SCORE_DOT);
    constexpr float L2E = 1.44269504088896340736f;
    constexpr int NCC = NCH / 2;     // 32-column chunks per wave
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* qn2 = reinterpret_cast<float*>(smem);
    float* qsc_s = qn2 + BQ;
    float* sn2 = qsc_s + BQ;
    float* ssc = sn2 + SBS;
    float* law = ssc + SBS;          // the tile's row log-weights (0 without them: the fused multiply-add is then exact)
    float4* stage = reinterpret_cast<float4*>(smem + S_HDR);
    _Float16* Wh = reinterpret_cast<_Float16*>(smem + S_HDR);
    _Float16* Wl = Wh + SBS * W_STRIDE;
    float* pmx = reinterpret_cast<float*>(smem + S_HDR);   // the W m exchange at the end, over the same bytes

    const int B = a.B, N = a.N, d = a.d, T = a.T;
    const int tid = threadIdx.x, lane = tid & 63, i = lane & 15, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // workgroup -> (chunk, support tile, slab): the workgroups that share a tile's bank rows are neighbours
    const int slab = blockIdx.x % a.nslabs, rest = blockIdx.x / a.nslabs;
    const int stile = rest % a.n_stiles, chunk = rest / a.n_stiles;
    const int s0 = stile * SBS;
    const int nk = d / BK, nkt = T / BK, ncb = T / 16;
    const int kc0 = slab * NCH;
    const int nc = min(NCH, nkt - kc0);                 // 32-column chunks of this slab
    const int qt_begin = chunk * a.tpc, qt_end = min(a.n_qtiles, qt_begin + a.tpc);
    const int rb = wave & 3, hf = wave >> 2;          // the third product: rows 16 rb .. + 15, chunks hf, hf + 2, ...
    const bool windowed = a.win_lo != nullptr;
    const bool weighted = a.row_logw != nullptr;
    const bool exclude = a.exclude != 0;
    const bool want_pm = a.want_glogw != 0 && slab == 0;

    for (int t = tid; t < SBS; t += TILE_THREADS) {
        const int j = min(s0 + t, N - 1);
        if (NEED_NORM) sn2[t] = a.s_norm2[j];
        ssc[t] = a.s_scale[j];
        law[t] = weighted ? a.row_logw[j] : 0.f;
    }
    __syncthreads();

    f32x4 gacc[NCC][2];
#pragma unroll
    for (int c = 0; c < NCC; ++c) gacc[c][0] = gacc[c][1] = f32x4{0.f, 0.f, 0.f, 0.f};
    float pm[SRS][4];
#pragma unroll
    for (int r = 0; r < SRS; ++r)
#pragma unroll
        for (int e = 0; e < 4; ++e) pm[r][e] = 0.f;
    float scale = 1.f;
    if (KIND == NW_SCORE_CLIP) scale = expf(*a.logit_scale);
    const int tile_end = s0 + SBS < N ? s0 + SBS : N;

    for (int qt = qt_begin; qt < qt_end; ++qt) {
        const int q0 = qt * BQ;
        f32x4 acc[SRS];
        tile_dots_f16x2<SRS, true>(a.q, a.s, B, N, d, q0, s0, stage, acc, qt % nk, qn2, qsc_s);
        __syncthreads();   // the ring is dead

        if (wave < NCONS) {
            // ================================ consumers: W, its m sums, its halves to LDS ================================
            using SF = ScoreFactors<KIND>;
            const int qrow = 16 * wave + i;
            const int b = q0 + qrow, bb = b < B ? b : B - 1;
            const float lse = a.lse[bb];
            // a dead query and a lane past B: W = 2^(u - inf) = 0 in every row
            const float lsev = (lse == -INFINITY || b >= B) ? INFINITY : lse * L2E;
            const float mq = a.ws.mb[bb];
            int lo = 0, hi = N;
            if (windowed) lo = min(max(a.win_lo[bb], 0), N), hi = min(max(a.win_hi[bb], 0), N);   // never used as addresses
            const unsigned width = hi > lo ? (unsigned)(hi - lo) : 0u;
            const float qn = NEED_NORM ? qn2[qrow] : 0.f;
            float Cq, Bq;
            SF::query(qn, qsc_s[qrow], scale, Cq, Bq);
            // the window's rule of the forward (fused_impl.h, OUT_WIN): a pair the window leaves whole skips the comparisons
            const bool whole = !windowed || (exclude ? (width == 0u || hi <= s0 || lo >= tile_end) : (lo <= s0 && hi >= tile_end));
            const bool check = !whole || tile_end < s0 + SBS || b >= B;
            const int rel = s0 + 4 * g - lo;
#pragma unroll
            for (int r = 0; r < SRS; ++r) {
                float4 n4 = make_float4(0.f, 0.f, 0.f, 0.f);
                if (NEED_NORM) n4 = *reinterpret_cast<const float4*>(sn2 + 16 * r + 4 * g);
                const float4 s4 = *reinterpret_cast<const float4*>(ssc + 16 * r + 4 * g);
                const float4 a4 = *reinterpret_cast<const float4*>(law + 16 * r + 4 * g);
                const float nn[4] = {n4.x, n4.y, n4.z, n4.w}, ss[4] = {s4.x, s4.y, s4.z, s4.w};
                const float aw[4] = {a4.x, a4.y, a4.z, a4.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float K, Base;
                    SF::support(nn[e], ss[e], K, Base);
                    const float u = SF::finish(__builtin_fmaf(acc[r][e], K * Cq, Base + Bq));   // base-2 units, as the forward
                    float W = __builtin_amdgcn_exp2f(__builtin_fmaf(aw[e], L2E, u) - lsev);
                    if (check) {
                        const int t = 16 * r + e;
                        bool keep = s0 + 4 * g + t < N && b < B;
                        if (windowed) keep = keep && (((unsigned)(rel + t) < width) != exclude);
                        W = keep ? W : 0.f;
                    }
                    pm[r][e] = __builtin_fmaf(W, mq, pm[r][e]);
                    const float x = __builtin_amdgcn_fmed3f(W * (float)(1 << W_SHIFT), 0.f, HALF_MAX);
                    const _Float16 h = (_Float16)x;
                    const int row = 16 * r + 4 * g + e;
                    Wh[row * W_STRIDE + qrow] = h;
                    Wl[row * W_STRIDE + qrow] = (_Float16)(x - (float)h);
                }
            }
        }
        __syncthreads();   // W is in LDS

        // ================================ all waves: gV tile += W^T G ================================
        {
            half8 Ah[2], Al[2];
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                Ah[ks] = *reinterpret_cast<const half8*>(Wh + (16 * rb + i) * W_STRIDE + 32 * ks + 8 * g);
                Al[ks] = *reinterpret_cast<const half8*>(Wl + (16 * rb + i) * W_STRIDE + 32 * ks + 8 * g);
            }
            auto mm = [](const half8& x, const half8& y, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(x, y, c, 0, 0, 0); };
            const half8* gq = a.ws.gpack + (size_t)qt * ncb * 256 + lane;
#pragma unroll
            for (int cc = 0; cc < NCC; ++cc) {
                const int c = 2 * cc + hf;
                if (c < nc) {
                    half8 Gf[2][2][2];   // [column block][step][h, l]
#pragma unroll
                    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
                        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                            for (int hl = 0; hl < 2; ++hl)
                                Gf[nb][ks][hl] = gq[((size_t)(2 * (kc0 + c) + nb) * 2 + ks) * 128 + hl * 64];
                    // small terms first, the dominant h*h product last; the two column blocks alternate
#pragma unroll
                    for (int ks = 0; ks < 2; ++ks) {
                        gacc[cc][0] = mm(Al[ks], Gf[0][ks][0], gacc[cc][0]);
                        gacc[cc][1] = mm(Al[ks], Gf[1][ks][0], gacc[cc][1]);
                        gacc[cc][0] = mm(Ah[ks], Gf[0][ks][1], gacc[cc][0]);
                        gacc[cc][1] = mm(Ah[ks], Gf[1][ks][1], gacc[cc][1]);
                        gacc[cc][0] = mm(Ah[ks], Gf[0][ks][0], gacc[cc][0]);
                        gacc[cc][1] = mm(Ah[ks], Gf[1][ks][0], gacc[cc][1]);
                    }
                }
            }
        }
        __syncthreads();   // the ring is free for the next tile
    }

    // ---- results: gacc[cc][nb][e] of lane (i, g) = gV'[row 16 rb + 4g + e][column 32 (kc0 + 2 cc + hf) + 16 nb + i]
    const int unshift = -(W_SHIFT + *a.ws.gexp);
    float dotp[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int cc = 0; cc < NCC; ++cc) {
        const int c = 2 * cc + hf;
        if (c < nc) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int row = s0 + 16 * rb + 4 * g + e;
                if (row < N) {
                    const size_t at = (size_t)row * T + (size_t)(kc0 + c) * BK + i;
                    const float g0 = __builtin_ldexpf(gacc[cc][0][e], unshift), g1 = __builtin_ldexpf(gacc[cc][1][e], unshift);
                    if (a.gv_out) {
                        float* dst = a.gv_out + (size_t)chunk * N * T + at;
                        dst[0] = g0;
                        dst[16] = g1;
                    }
                    if (a.want_glogw) {
                        dotp[e] = __builtin_fmaf(g0, a.v_rows[at], dotp[e]);
                        dotp[e] = __builtin_fmaf(g1, a.v_rows[at + 16], dotp[e]);
                    }
                }
            }
        }
    }
    if (a.want_glogw) {
        const size_t npad = (size_t)a.n_stiles * SBS;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float v = dotp[e];
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o);   // the 16 lanes of a row: a fixed tree
            if (i == 0)
                a.ws.glp[((size_t)chunk * a.nslabs * 2 + 2 * slab + hf) * npad + s0 + 16 * rb + 4 * g + e] = v;
        }
        if (want_pm) {   // (uniform over the workgroup)
            if (wave < NCONS) {
#pragma unroll
                for (int r = 0; r < SRS; ++r)
#pragma unroll
                    for (int e = 0; e < 4; ++e) pmx[(16 * wave + i) * SBS + 16 * r + 4 * g + e] = pm[r][e];
            }
            __syncthreads();
            if (tid < SBS) {
                float v = 0.f;
                for (int k = 0; k < BQ; ++k) v += pmx[k * SBS + tid];   // the tile's 64 query slots in order
                a.ws.pmp[(size_t)chunk * npad + s0 + tid] = v;
            }
        }
    }
}

// glogw[j] = sum_chunks sum_(slab, half) glp - sum_chunks pmp, each in ascending order from +0
__global__ __launch_bounds__(256) void nw_bwd_values_support_glogw_kernel(const float* __restrict__ glp, const float* __restrict__ pmp,
                                                                           float* __restrict__ glogw, int nparts, int nchunks,
                                                                           int64_t npad, int64_t N) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= N) return;
    float v = 0.f, m = 0.f;
    for (int p = 0; p < nparts; ++p) v += glp[(int64_t)p * npad + j];
    for (int c = 0; c < nchunks; ++c) m += pmp[(int64_t)c * npad + j];
    glogw[j] = v - m;
}

// gvalues = sum_chunks part[c], chunks in order (float4s)
__global__ __launch_bounds__(256) void nw_bwd_values_support_finish_kernel(const float* __restrict__ part, float* __restrict__ gvalues,
                                                                            int nchunks, int64_t total4) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total4) return;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int c = 0; c < nchunks; ++c) {
        const float4 w = *reinterpret_cast<const float4*>(part + ((int64_t)c * total4 + idx) * 4);
        v.x += w.x; v.y += w.y; v.z += w.z; v.w += w.w;
    }
    *reinterpret_cast<float4*>(gvalues + idx * 4) = v;
}

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// Slab width: the narrow one when it takes all of T.  Query chunks: one when the support tiles and slabs alone fill the
// chip, otherwise as many as do (at most the query tiles); a positive query_chunks is taken, clamped to the query tiles.
SupPlan sup_plan(int64_t B, int64_t N, int64_t T, int query_chunks) {
    const int64_t n_stiles = (N + SBS - 1) / SBS, n_qtiles = (B + BQ - 1) / BQ, nkt = T / BK;
    const int nch = nkt <= S_NCH_MIN ? S_NCH_MIN : S_NCH_MAX;
    const int64_t nslabs = (nkt + nch - 1) / nch;
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

// mb | gmax | gexp | gpack | glp | pmp | part
size_t sup_layout(int64_t B, int64_t N, int64_t T, const SupPlan& p, bool want_gvalues, char* base, SupWs* ws) {
    size_t off = 0;
    auto take = [&](size_t bytes) {
        char* ptr = base ? base + off : nullptr;
        off += align256(bytes);
        return ptr;
    };
    const size_t npad = (size_t)p.n_stiles * SBS;
    SupWs w;
    w.mb = reinterpret_cast<float*>(take((size_t)B * 4));
    w.gmax = reinterpret_cast<float*>(take((size_t)B * 4));
    w.gexp = reinterpret_cast<int*>(take(4));
    w.gpack = reinterpret_cast<half8*>(take((size_t)p.n_qtiles * BQ * T * 4));
    // (the weights' partial sums are laid out whether or not glogw is asked for: the size depends on the shape alone)
    w.glp = reinterpret_cast<float*>(take((size_t)p.nchunks * p.nslabs * 2 * npad * 4));
    w.pmp = reinterpret_cast<float*>(take((size_t)p.nchunks * npad * 4));
    w.part = reinterpret_cast<float*>(take(want_gvalues && p.nchunks > 1 ? (size_t)p.nchunks * N * T * 4 : 0));
    if (ws) *ws = w;
    return off;
}

template <int KIND, int NCH>
int launch_sup_kernel(const SupArgs& a, unsigned grid, hipStream_t st) {
    static const bool attr = hipFuncSetAttribute(reinterpret_cast<const void*>(nw_bwd_values_support_kernel<KIND, NCH>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)S_LDS) == hipSuccess;
    if (!attr) return NW_ERR_LAUNCH;
    hipLaunchKernelGGL((nw_bwd_values_support_kernel<KIND, NCH>), dim3(grid), dim3(TILE_THREADS), S_LDS, st, a);
    return NW_OK;
}
template <int KIND>
int launch_sup_kind(const SupArgs& a, int nch, unsigned grid, hipStream_t st) {
    if (nch == S_NCH_MAX) return launch_sup_kernel<KIND, S_NCH_MAX>(a, grid, st);
    return launch_sup_kernel<KIND, S_NCH_MIN>(a, grid, st);
}

}  // namespace

size_t bwd_values_support_workspace_bytes(int64_t B, int64_t N, int64_t d, int64_t T, int query_chunks, bool want_gvalues) {
    if (B <= 0 || !fwd_values_shape_ok(B, N, d, T)) return 0;
    return sup_layout(B, N, T, sup_plan(B, N, T, query_chunks), want_gvalues, nullptr, nullptr);
}

int launch_bwd_values_support(const BwdValuesSupportCall& c) {
    hipStream_t st = c.st;
    const SupPlan p = sup_plan(c.B, c.N, c.T, c.query_chunks);
    SupWs ws;
    const size_t need = sup_layout(c.B, c.N, c.T, p, c.gvalues != nullptr, static_cast<char*>(c.workspace), &ws);
    if (!c.workspace || c.workspace_bytes < need) return NW_ERR_WORKSPACE;
    const int64_t wgs = (int64_t)p.n_stiles * p.nslabs * p.nchunks;
    const int64_t npack = (int64_t)p.n_qtiles * (c.T / 16) * 128, total4 = c.N * c.T / 4;
    if (wgs > 0x7fffffffLL || (npack + 255) / 256 > 0x7fffffffLL || (total4 + 255) / 256 > 0x7fffffffLL) return NW_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(nw_bwd_values_support_prologue_kernel, dim3((unsigned)c.B), dim3(256), 0, st, c.out, c.gout, ws.mb, ws.gmax,
                       c.T);
    hipLaunchKernelGGL(nw_bwd_values_support_gexp_kernel, dim3(1), dim3(256), 0, st, ws.gmax, ws.gexp, c.B);
    hipLaunchKernelGGL(nw_bwd_values_support_pack_kernel, dim3((unsigned)((npack + 255) / 256)), dim3(256), 0, st, c.gout, ws.gexp,
                       ws.gpack, c.B, c.T, npack);
    float* gv_out = c.gvalues ? (p.nchunks > 1 ? ws.part : c.gvalues) : nullptr;
    const SupArgs a = {c.q, c.s_split, c.s_scale, c.s_norm2, c.v_rows, c.row_lo, c.row_hi, c.lse, c.logit_scale_dev, c.row_logw,
                       gv_out, ws, c.glogw != nullptr, c.row_lo && c.exclude != 0, (int)c.B, (int)c.N, (int)c.d, (int)c.T,
                       p.n_stiles, p.n_qtiles, p.nslabs, p.nchunks, p.tpc};
    int rc;
    switch (c.kind) {
        case NW_SCORE_EUCLIDEAN: rc = launch_sup_kind<NW_SCORE_EUCLIDEAN>(a, p.nch, (unsigned)wgs, st); break;
        case NW_SCORE_HYPERSPHERE: rc = launch_sup_kind<NW_SCORE_HYPERSPHERE>(a, p.nch, (unsigned)wgs, st); break;
        case NW_SCORE_COSINE: rc = launch_sup_kind<NW_SCORE_COSINE>(a, p.nch, (unsigned)wgs, st); break;
        case NW_SCORE_DOT: rc = launch_sup_kind<NW_SCORE_DOT>(a, p.nch, (unsigned)wgs, st); break;
        default: rc = launch_sup_kind<NW_SCORE_CLIP>(a, p.nch, (unsigned)wgs, st); break;
    }
    if (rc != NW_OK) return rc;
    if (c.gvalues && p.nchunks > 1)
        hipLaunchKernelGGL(nw_bwd_values_support_finish_kernel, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, st, ws.part,
                           c.gvalues, p.nchunks, total4);
    if (c.glogw)
        hipLaunchKernelGGL(nw_bwd_values_support_glogw_kernel, dim3((unsigned)((c.N + 255) / 256)), dim3(256), 0, st, ws.glp, ws.pmp,
                           c.glogw, p.nchunks * p.nslabs * 2, p.nchunks, (int64_t)p.n_stiles * SBS, c.N);
    NW_CHECK_LAUNCH();
    return NW_OK;
}

}  // namespace nw
