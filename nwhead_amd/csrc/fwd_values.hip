// fwd_values.hip -- the VALUE head over a resident split bank: Nadaraya-Watson regression with a real-valued target row
// per support, without a (B,N) matrix (gfx950 / MI355X only; nw_fwd_values_f32).
//
//     out[b,t] = sum_{j admitted} W_bj v_jt,     W_bj = exp(score_bj + a_j - lse_b)
// with lse_b the log-sum-exp of a first pass over the same operands (nw_fwd_window_f32 / nw_fwd_weighted_f32 with lse_out),
// the window and the row weights a_j those of nw_bwd_query_weighted_f32.  The skeleton is bwd_query.hip's: a workgroup owns
// 64 queries, a contiguous chunk of 64-row support tiles and a slab of 32 * NCH columns -- here columns of T.  Per tile it
//   1. recomputes the tile's dot products like the forward does (tile_dots_f16x2);
//   2. turns them into W in registers (score, the forward's fused multiply-add for the weight, the window's rule; an exact
//      0 for a row at a = -inf, a row outside the window, a clamped row past N and every row of a dead query), scales the
//      row by 2^E_b and the element by the value row's 2^-e_j, and splits it into fp16 halves;
//   3. streams the tile's VALUE rows (split rows of nw_split_rows_f16x2, (N,T)), 32 columns at a time, and adds W' v' to its
//      64 x (32 NCH) accumulators on v_mfma_f32_16x16x32_f16 (lh, hl, hh), the value operand read with ds_read_b64_tr_b16
//      (the layouts are spelled out in bwd_query.hip's header).
// Scaling: v'_j = v_j 2^e_j are the value rows; W'_bj = W_bj 2^-e_j 2^E with ONE running power-of-two exponent per query
// row and chunk, raised when a tile shows a larger coefficient, the row's accumulators rescaled by the exact power of two
// between the old and the new one.  W alone is at most 1, but 2^-e_j spans the values' magnitudes.
// The value rows must be FINITE in every row, admitted or not: the coefficient of a row that takes no part is an exact 0,
// and 0 x inf is NaN on the matrix pipe.
//
// Chunks over N fill the chip; each writes its partial (B,T) tile and its row exponents, nw_fwd_values_finish_kernel adds
// them in chunk order: no float atomics, two calls give the same bits.
#include "nw_internal.h"
#include "tile_dma.h"
#include "tile_f16.h"

namespace nw {
namespace {

typedef __fp16 fp16x4 __attribute__((__vector_size__(4 * sizeof(__fp16))));
typedef _Float16 halfx4 __attribute__((ext_vector_type(4)));

constexpr int VRS = 4;            // support blocks per tile
constexpr int VBS = 16 * VRS;     // 64 bank rows per tile
// qn2[BQ] | qsc[BQ] | fac[BQ] | sn2[VBS] | ssc[VBS] | vsc[VBS] | law[VBS]
constexpr int V_HDR = (3 * BQ + 4 * VBS) * 4;
static_assert(V_HDR % 16 == 0, "stage buffers must stay 16-byte aligned");
constexpr size_t V_LDS = V_HDR + DmaCfg<VRS>::STAGE_BYTES;
static_assert(V_LDS <= 80 * 1024, "header + ring exceed the LDS of two workgroups per CU");
// the second product's ring (over the forward's, dead by then): 64 rows x 128 B per stage
constexpr int V2_STAGE = VBS * 128, V2_NBUF = 4, V2_NI = VBS / 8 / NLOAD;
static_assert((size_t)V2_NBUF * V2_STAGE <= DmaCfg<VRS>::STAGE_BYTES, "second ring inside the first");
constexpr int V_CUS = 256;        // workgroups that fill the chip
constexpr float HALF_MAX = 60000.f;

struct FwdValuesPlan {
    int n_stiles, n_qtiles, nch, nslabs, nchunks, tpc;
};
struct FwdValuesArgs {
    const float *q, *s, *s_scale, *s_norm2, *v, *v_scale;
    const int *win_lo, *win_hi;
    const float *lse, *logit_scale, *row_logw;
    float *ascale, *part;
    int exclude, B, N, d, T, n_stiles, n_qtiles, nslabs, nchunks, tpc;
};

template <int KIND, int NCH>
__global__ __launch_bounds__(TILE_THREADS, 2) void nw_fwd_values_kernel(const FwdValuesArgs a) {
    constexpr bool NEED_NORM = (KIND != NW_SCORE_DOT);
    constexpr float L2E = 1.44269504088896340736f;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* qn2 = reinterpret_cast<float*>(smem);
    float* qsc_s = qn2 + BQ;
    float* fac_s = qsc_s + BQ;       // rescaling factors of the rows, wave-private
    float* sn2 = fac_s + BQ;
    float* ssc = sn2 + VBS;
    float* vsc = ssc + VBS;          // the value rows' 2^-e_j
    float* law = vsc + VBS;          // the tile's row log-weights (0 without them: the fused multiply-add is then exact)
    float4* stage = reinterpret_cast<float4*>(smem + V_HDR);
    const char* ring2 = smem + V_HDR;

    const int B = a.B, N = a.N, d = a.d, T = a.T;
    const int tid = threadIdx.x, lane = tid & 63, i = lane & 15, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // workgroup -> (chunk, slab, query tile): the workgroups that share a chunk's bank rows are neighbours
    const int qt = blockIdx.x % a.n_qtiles, rest = blockIdx.x / a.n_qtiles;
    const int slab = rest % a.nslabs, chunk = rest / a.nslabs;
    const int q0 = qt * BQ;
    const int nk = d / BK, nkt = T / BK;
    const int kc0 = slab * NCH;
    const int nc = min(NCH, nkt - kc0);                // 32-column blocks of this slab
    const int st_begin = chunk * a.tpc, st_end = min(a.n_stiles, st_begin + a.tpc);

    // ---- what a consumer lane knows of its query (query 16 wave + i on the lane)
    const int qrow = 16 * (wave & 3) + i;
    const int b = q0 + qrow, bb = b < B ? b : B - 1;
    const float lse = a.lse[bb];
    const float lsev = lse == -INFINITY ? INFINITY : lse * L2E;   // a dead query: W = 2^(u - inf) = 0 in every row
    const bool windowed = a.win_lo != nullptr;
    const bool weighted = a.row_logw != nullptr;
    int lo = 0, hi = N;
    if (windowed) lo = min(max(a.win_lo[bb], 0), N), hi = min(max(a.win_hi[bb], 0), N);   // never used as addresses
    const unsigned width = hi > lo ? (unsigned)(hi - lo) : 0u;
    const bool exclude = a.exclude != 0;

    f32x4 oacc[NCH][2];
#pragma unroll
    for (int c = 0; c < NCH; ++c) oacc[c][0] = oacc[c][1] = f32x4{0.f, 0.f, 0.f, 0.f};
    int Erun = 0;          // the row's exponent in this chunk so far; `have`: some tile has set it
    bool have = false;

    // transposed reads of the second product (bwd_query.hip): lane 4q + p of group g supplies row 4g + q (+ 16h + 32t),
    // bytes 8(p & 1) of 16-byte slot (gs + (p >> 1)) ^ sw, sw = 2 ((row >> 1) & 3)
    const int tq4 = i >> 2, tp = i & 3;
    const int sw2 = ((2 * g + (tq4 >> 1)) & 3) << 1;
    const int trow = (4 * g + tq4) * 128 + 8 * (tp & 1);
    int toff[2][2];   // [half: h, l][16-column block]
#pragma unroll
    for (int hl = 0; hl < 2; ++hl)
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) toff[hl][nb] = trow + (((4 * hl + 2 * nb + (tp >> 1)) ^ sw2) << 4);

    for (int st = st_begin; st < st_end; ++st) {
        const int s0 = st * VBS;
        for (int t = tid; t < VBS; t += TILE_THREADS) {
            const int j = min(s0 + t, N - 1);
            if (NEED_NORM) sn2[t] = a.s_norm2[j];
            ssc[t] = a.s_scale[j];
            vsc[t] = a.v_scale[j];
            law[t] = weighted ? a.row_logw[j] : 0.f;
        }
        f32x4 acc[VRS];
        tile_dots_f16x2<VRS, true>(a.q, a.s, B, N, d, q0, s0, stage, acc, st % nk, qn2, qsc_s);
        __syncthreads();   // the header is visible, the ring is dead

        if (wave < NCONS) {
            // ================================ consumers: W' in registers ================================
            half8 Ah[VRS / 2], Al[VRS / 2];
            {
                using SF = ScoreFactors<KIND>;
                const float qn = NEED_NORM ? qn2[qrow] : 0.f;
                float scale = 1.f;
                if (KIND == NW_SCORE_CLIP) scale = expf(*a.logit_scale);
                float Cq, Bq;
                SF::query(qn, qsc_s[qrow], scale, Cq, Bq);
                const int tile_end = s0 + VBS < N ? s0 + VBS : N;
                // the window's rule of the forward (fused_impl.h, OUT_WIN): a pair the window leaves whole skips the comparisons
                const bool whole = !windowed || (exclude ? (width == 0u || hi <= s0 || lo >= tile_end) : (lo <= s0 && hi >= tile_end));
                const bool check = !whole || tile_end < s0 + VBS;
                const int rel = s0 + 4 * g - lo;
                float xr[VRS][4], amax = 0.f;
#pragma unroll
                for (int r = 0; r < VRS; ++r) {
                    float4 n4 = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (NEED_NORM) n4 = *reinterpret_cast<const float4*>(sn2 + 16 * r + 4 * g);
                    const float4 s4 = *reinterpret_cast<const float4*>(ssc + 16 * r + 4 * g);
                    const float4 v4 = *reinterpret_cast<const float4*>(vsc + 16 * r + 4 * g);
                    const float4 a4 = *reinterpret_cast<const float4*>(law + 16 * r + 4 * g);
                    const float nn[4] = {n4.x, n4.y, n4.z, n4.w}, ss[4] = {s4.x, s4.y, s4.z, s4.w};
                    const float vs[4] = {v4.x, v4.y, v4.z, v4.w}, aw[4] = {a4.x, a4.y, a4.z, a4.w};
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        float K, Base;
                        SF::support(nn[e], ss[e], K, Base);
                        const float u = SF::finish(__builtin_fmaf(acc[r][e], K * Cq, Base + Bq));   // base-2 units, as the forward
                        float W = __builtin_amdgcn_exp2f(__builtin_fmaf(aw[e], L2E, u) - lsev);    // the forward's fused multiply-add
                        if (check) {
                            const int t = 16 * r + e;
                            bool keep = s0 + 4 * g + t < N;
                            if (windowed) keep = keep && (((unsigned)(rel + t) < width) != exclude);
                            W = keep ? W : 0.f;
                        }
                        xr[r][e] = W * vs[e];
                        amax = fmaxf(amax, fabsf(xr[r][e]));
                    }
                }
                // the row's exponent: raised (a smaller E) when this tile holds a larger coefficient than any before it
                amax = group4_max(amax);
                float factor = 1.f;
                if (amax > 0.f && amax < INFINITY) {
                    const int En = split_exponent(amax);
                    if (!have || En < Erun) {
                        if (have) factor = __builtin_ldexpf(1.f, En - Erun);   // (before: the row's accumulators are all zero)
                        Erun = En;
                        have = true;
                    }
                }
                const float up = __builtin_ldexpf(1.f, Erun);
#pragma unroll
                for (int r = 0; r < VRS; ++r)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float x = __builtin_amdgcn_fmed3f(xr[r][e] * up, -HALF_MAX, HALF_MAX);   // (only a non-finite input gets here)
                        const _Float16 h = (_Float16)x;
                        Ah[r >> 1][4 * (r & 1) + e] = h;
                        Al[r >> 1][4 * (r & 1) + e] = (_Float16)(x - (float)h);
                    }
                // lane (i, g) holds the accumulators of queries 4g + e: their factors come from the lanes that own them.  A
                // wave's LDS operations execute in order and the 16 floats are this wave's own: no barrier
                if (g == 0) fac_s[qrow] = factor;
                __builtin_amdgcn_wave_barrier();
                asm volatile("" ::: "memory");
                if (__any(factor != 1.f)) {
                    const float4 f4 = *reinterpret_cast<const float4*>(fac_s + 16 * (wave & 3) + 4 * g);
                    const f32x4 fv = {f4.x, f4.y, f4.z, f4.w};
#pragma unroll
                    for (int c = 0; c < NCH; ++c) {
                        oacc[c][0] *= fv;
                        oacc[c][1] *= fv;
                    }
                }
            }
            // ================================ consumers: out tile += W' v' ================================
            auto tr8 = [&](const char* base, int off) {
                const halfx4 v0 = __builtin_bit_cast(halfx4, __builtin_amdgcn_ds_read_tr16_b64_v4f16(
                    (__attribute__((address_space(3))) fp16x4*)(base + off)));
                const halfx4 v1 = __builtin_bit_cast(halfx4, __builtin_amdgcn_ds_read_tr16_b64_v4f16(
                    (__attribute__((address_space(3))) fp16x4*)(base + off + 16 * 128)));
                return half8{v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
            };
            auto mm = [](const half8& x, const half8& y, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(x, y, c, 0, 0, 0); };
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
                if (c < nc) {
                    tile_barrier();   // stage c has landed
                    const char* buf = ring2 + (c % V2_NBUF) * V2_STAGE;
#pragma unroll
                    for (int t = 0; t < VRS / 2; ++t) {
                        const half8 bh0 = tr8(buf, toff[0][0] + 32 * 128 * t), bh1 = tr8(buf, toff[0][1] + 32 * 128 * t);
                        const half8 bl0 = tr8(buf, toff[1][0] + 32 * 128 * t), bl1 = tr8(buf, toff[1][1] + 32 * 128 * t);
                        // small terms first, the dominant h*h product last; the two column blocks alternate
                        oacc[c][0] = mm(Al[t], bh0, oacc[c][0]);
                        oacc[c][1] = mm(Al[t], bh1, oacc[c][1]);
                        oacc[c][0] = mm(Ah[t], bl0, oacc[c][0]);
                        oacc[c][1] = mm(Ah[t], bl1, oacc[c][1]);
                        oacc[c][0] = mm(Ah[t], bh0, oacc[c][0]);
                        oacc[c][1] = mm(Ah[t], bh1, oacc[c][1]);
                    }
                }
            }
            tile_barrier();   // the ring is free for the next tile
        } else {
            // ================================ loaders: the tile's value rows, this slab's columns ================================
            const int lw = wave - NCONS;
            unsigned voff[V2_NI];
#pragma unroll
            for (int m = 0; m < V2_NI; ++m) {
                const int R = 8 * (lw + NLOAD * m) + (lane >> 3);
                const int lslot = (lane & 7) ^ (((R >> 1) & 3) << 1);   // source-side swizzle (see toff)
                const int rel = min(s0 + R, N - 1) - s0;                // a row past N repeats row N - 1: its coefficient is 0
                voff[m] = ((unsigned)rel * (unsigned)T + lslot * 4) * 4u;
            }
            const char* sb = reinterpret_cast<const char*>(a.v + (size_t)s0 * T) + (size_t)kc0 * BK * 4;
            auto issue = [&](int c) {
                char* buf = smem + V_HDR + (c % V2_NBUF) * V2_STAGE;
#pragma unroll
                for (int m = 0; m < V2_NI; ++m)
                    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(sb + (size_t)c * BK * 4 + voff[m]),
                                                     (__attribute__((address_space(3))) void*)(buf + 1024 * (lw + NLOAD * m)), 16, 0, 0);
            };
            constexpr int AHEAD = V2_NBUF - 1;
#pragma unroll
            for (int c = 0; c < AHEAD; ++c)
                if (c < nc) issue(c);
            for (int c = 0; c < nc; ++c) {
                if (c + AHEAD <= nc) wait_vmcnt<(AHEAD - 1) * V2_NI>(); else wait_vmcnt<0>();
                tile_barrier();   // stage c is published; the consumers have left stage c - 1
                if (c + AHEAD < nc) issue(c + AHEAD);
            }
            tile_barrier();
        }
    }

    if (wave >= NCONS) return;
    // ---- partial results of this chunk: oacc[c][nb][e] of lane (i, g) = out'[query 16 wave + 4g + e][column 32 (kc0 + c) + 16 nb + i]
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        if (c < nc) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int bo = q0 + 16 * wave + 4 * g + e;
                if (bo < B) {
                    float* row = a.part + ((size_t)chunk * B + bo) * T + (size_t)(kc0 + c) * BK + i;
                    row[0] = oacc[c][0][e];
                    row[16] = oacc[c][1][e];
                }
            }
        }
    }
    // (1 when no tile set the exponent: the partial row is zero)
    if (slab == 0 && g == 0 && b < B) a.ascale[(size_t)chunk * B + b] = __builtin_ldexpf(1.f, -Erun);
}

// out[b,t] = sum_chunks 2^-E[c][b] part[c][b,t], chunks in order (t in float4s)
__global__ __launch_bounds__(256) void nw_fwd_values_finish_kernel(const float* __restrict__ part, const float* __restrict__ ascale,
                                                                    float* __restrict__ out, int nchunks, int64_t B, int64_t T) {
    const int64_t total4 = B * T / 4;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total4) return;
    const int64_t b = (idx * 4) / T;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int c = 0; c < nchunks; ++c) {
        const float4 w = *reinterpret_cast<const float4*>(part + (int64_t)c * B * T + idx * 4);
        const float f = ascale[(int64_t)c * B + b];   // a power of two: exact
        v.x += w.x * f; v.y += w.y * f; v.z += w.z * f; v.w += w.w * f;
    }
    *reinterpret_cast<float4*>(out + idx * 4) = v;
}

// Slab width and chunk count, by bwd_query_plan's model with T in d's place for the second product: per support tile a
// workgroup costs 3 d/32 for the scores (every slab recomputes them) + 4 per 32 columns of its slab; the grid runs in
// ceil(workgroups / CUs) rounds.  The library's own choice keeps the partial tiles, nchunks B T 4 bytes, below 0.85 B N
// bytes (a fifth of one score matrix).
FwdValuesPlan fwd_values_plan(int64_t B, int64_t N, int64_t d, int64_t T, int row_chunks) {
    FwdValuesPlan best = {};
    const int64_t n_stiles = (N + VBS - 1) / VBS, n_qtiles = (B + BQ - 1) / BQ, nk = d / BK, nkt = T / BK;
    int64_t best_cost = -1;
    for (int nch = 8; nch >= 4; nch >>= 1) {
        if (nch > 4 && nch / 2 >= nkt) continue;   // a narrower slab already takes the whole width
        const int64_t nslabs = (nkt + nch - 1) / nch;
        int64_t want;
        if (row_chunks > 0) {
            want = row_chunks < n_stiles ? row_chunks : n_stiles;
        } else {
            const int64_t fit = n_stiles * VBS * 27 / (128 * T), cap = fit > 1 ? fit : 1;
            want = (V_CUS + n_qtiles * nslabs - 1) / (n_qtiles * nslabs);
            if (want > cap) want = cap;
        }
        const int64_t tpc = (n_stiles + want - 1) / want, nchunks = (n_stiles + tpc - 1) / tpc;
        const int64_t wgs = n_qtiles * nslabs * nchunks, rounds = (wgs + V_CUS - 1) / V_CUS;
        const int64_t cost = rounds * tpc * (3 * nk + 4 * (nch < nkt ? nch : nkt));
        if (best_cost < 0 || cost < best_cost) {
            best_cost = cost;
            best = {(int)n_stiles, (int)n_qtiles, nch, (int)nslabs, (int)nchunks, (int)tpc};
        }
    }
    return best;
}

// ascale | part
size_t fwd_values_layout(int64_t B, int64_t T, const FwdValuesPlan& p, char* base, float** ascale, float** part) {
    const size_t a_bytes = align256((size_t)p.nchunks * B * sizeof(float));
    const size_t p_bytes = align256((size_t)p.nchunks * B * T * sizeof(float));
    if (ascale) *ascale = base ? reinterpret_cast<float*>(base) : nullptr;
    if (part) *part = base ? reinterpret_cast<float*>(base + a_bytes) : nullptr;
    return a_bytes + p_bytes;
}

template <int KIND, int NCH>
int launch_fwd_values_kernel(const FwdValuesArgs& a, unsigned grid, hipStream_t st) {
    static const bool attr = hipFuncSetAttribute(reinterpret_cast<const void*>(nw_fwd_values_kernel<KIND, NCH>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)V_LDS) == hipSuccess;
    if (!attr) return NW_ERR_LAUNCH;
    hipLaunchKernelGGL((nw_fwd_values_kernel<KIND, NCH>), dim3(grid), dim3(TILE_THREADS), V_LDS, st, a);
    return NW_OK;
}
template <int KIND>
int launch_fwd_values_kind(const FwdValuesArgs& a, int nch, unsigned grid, hipStream_t st) {
    return nch == 8 ? launch_fwd_values_kernel<KIND, 8>(a, grid, st) : launch_fwd_values_kernel<KIND, 4>(a, grid, st);
}

}  // namespace

bool fwd_values_shape_ok(int64_t B, int64_t N, int64_t d, int64_t T) {
    return bank_head_shape_ok(N, d, 1) && T >= 32 && T % 32 == 0 && T <= 16384 && B <= 0x7fffffffLL - BQ &&
           N <= 0x7fffffffLL - VBS;
}

size_t fwd_values_workspace_bytes(int64_t B, int64_t N, int64_t d, int64_t T, int row_chunks) {
    if (B <= 0 || !fwd_values_shape_ok(B, N, d, T)) return 0;
    return fwd_values_layout(B, T, fwd_values_plan(B, N, d, T, row_chunks), nullptr, nullptr, nullptr);
}

int launch_fwd_values(const FwdValuesCall& c) {
    hipStream_t st = c.st;
    const FwdValuesPlan p = fwd_values_plan(c.B, c.N, c.d, c.T, c.row_chunks);
    float *ascale, *part;
    const size_t need = fwd_values_layout(c.B, c.T, p, static_cast<char*>(c.workspace), &ascale, &part);
    if (!c.workspace || c.workspace_bytes < need) return NW_ERR_WORKSPACE;
    const int64_t wgs = (int64_t)p.n_qtiles * p.nslabs * p.nchunks;
    if (wgs > 0x7fffffffLL || (c.B * c.T / 4 + 255) / 256 > 0x7fffffffLL) return NW_ERR_UNSUPPORTED;
    const FwdValuesArgs a = {c.q, c.s_split, c.s_scale, c.s_norm2, c.v_split, c.v_scale, c.row_lo, c.row_hi, c.lse,
                             c.logit_scale_dev, c.row_logw, ascale, part, c.row_lo && c.exclude != 0, (int)c.B, (int)c.N, (int)c.d,
                             (int)c.T, p.n_stiles, p.n_qtiles, p.nslabs, p.nchunks, p.tpc};
    int rc;
    switch (c.kind) {
        case NW_SCORE_EUCLIDEAN: rc = launch_fwd_values_kind<NW_SCORE_EUCLIDEAN>(a, p.nch, (unsigned)wgs, st); break;
        case NW_SCORE_HYPERSPHERE: rc = launch_fwd_values_kind<NW_SCORE_HYPERSPHERE>(a, p.nch, (unsigned)wgs, st); break;
        case NW_SCORE_COSINE: rc = launch_fwd_values_kind<NW_SCORE_COSINE>(a, p.nch, (unsigned)wgs, st); break;
        case NW_SCORE_DOT: rc = launch_fwd_values_kind<NW_SCORE_DOT>(a, p.nch, (unsigned)wgs, st); break;
        default: rc = launch_fwd_values_kind<NW_SCORE_CLIP>(a, p.nch, (unsigned)wgs, st); break;
    }
    if (rc != NW_OK) return rc;
    hipLaunchKernelGGL(nw_fwd_values_finish_kernel, dim3((unsigned)((c.B * c.T / 4 + 255) / 256)), dim3(256), 0, st, part, ascale,
                       c.out, p.nchunks, c.B, c.T);
    NW_CHECK_LAUNCH();
    return NW_OK;
}

}  // namespace nw
