// bwd_values.hip -- gradient of the VALUE head w.r.t. the queries over a resident split bank, without a (B,N) matrix
// (gfx950 / MI355X only; nw_bwd_values_query_f32).
//
// The forward (fwd_values.hip) is out_b = sum_j W_bj v_j, W_bj = exp(score_bj + a_j - lse_b) on the rows the window admits
// and 0 elsewhere.  With g the (B,T) upstream gradient and the bank, the values and the weights constants:
//     c_bj = g_b . v_j          (a T-long dot product: the second matrix product G V^T)
//     m_b  = g_b . out_b        (B floats, a prologue)
//     dS_bj = W_bj (c_bj - m_b)
//     A_bj = dS_bj df/ddot     rq_b = sum_j dS_bj df/d|q|^2     gls = sum_bj dS_bj df/dlogit_scale   (bwd_coeff.h)
//     gq_b = sum_j A_bj s_j + 2 rq_b q_b
// i.e. bwd_query.hip with its table lookups dW_j = dP[y_j] and t_b replaced by c_bj and m_b.  The weights a_j enter W only;
// the derivatives are taken at the raw score, as in the weighted class head.
//
// The skeleton is bwd_query.hip's: a workgroup owns 64 queries, a contiguous chunk of 64-row support tiles and a slab of
// 32 * NCH columns of d.  Per support tile it
//   1. recomputes the tile's dot products like the forward does (tile_dots_f16x2 over q, the split bank rows, d);
//   2. computes c with the same routine over (gout, the split value rows, T) on the same ring, behind a barrier (the ring
//      of the first product must be dead).  The raw gout rows are split in registers by the routine's own per-row exponent,
//      like raw queries; its row statistics go to header arrays of their own (gsc, gn2), beside the query's.  The
//      accumulator layout of both products is the same -- query on the lane, rows 16r + 4g + e in the registers -- so
//      c = acc2 gsc_b vsc_j meets W element for element with no exchange;
//   3. forms dS = W (c - m_b) with the forward's window rule and fused multiply-add for the weight, the kind's derivative
//      (bwd_pair_coeff), the running power-of-two row exponent with its exact rescale of the accumulators, fp16 halves;
//   4. streams the tile's bank rows once more, 32 columns at a time, and adds A' s' to its 64 x (32 NCH) accumulators on
//      v_mfma_f32_16x16x32_f16 (lh, hl, hh), exactly as bwd_query.hip does (its header spells the layouts out).
// Exact zeros: a dead query (lse = -inf: W = 0 in every row, m = 0), a row outside the window, a row at a = -inf, a clamped
// row past N and a lane past B contribute exactly 0.  The value rows must be FINITE in every row, the forward's condition:
// c of a row that takes no part is multiplied with W = 0.
// Scaling a row of gout by 2^k scales its row of gq exactly: gsc_b and m_b follow it, acc2 does not move.
//
// Accuracy.  c - m cancels: the error of c is ~2.4e-7 sum_t |g_t v_jt| (tile_f16.h), whatever the spread of the values
// among the rows, so values with a large common offset lose that many bits of the gradient.  Centre such columns.
//
// Chunks over N fill the chip; each writes its partial gq / rq / gls and its row exponents, the finish kernels add them in
// chunk order: no float atomics, two calls give the same bits.
#include "nw_internal.h"
#include "tile_dma.h"
#include "tile_f16.h"
#include "bwd_coeff.h"

namespace nw {
namespace {

typedef __fp16 fp16x4 __attribute__((__vector_size__(4 * sizeof(__fp16))));
typedef _Float16 halfx4 __attribute__((ext_vector_type(4)));

constexpr int GRS = 4;            // support blocks per tile
constexpr int GBS = 16 * GRS;     // 64 bank rows per tile
// qn2[BQ] | qsc[BQ] | fac[BQ] | gn2[BQ] | gsc[BQ] | sn2[GBS] | ssc[GBS] | vsc[GBS] | law[GBS]
constexpr int G_HDR = (5 * BQ + 4 * GBS) * 4;
static_assert(G_HDR % 16 == 0, "stage buffers must stay 16-byte aligned");
constexpr size_t G_LDS = G_HDR + DmaCfg<GRS>::STAGE_BYTES;
static_assert(G_LDS <= 80 * 1024, "header + ring exceed the LDS of two workgroups per CU");
// the third product's ring (over the first two's, dead by then): 64 rows x 128 B per stage
constexpr int G2_STAGE = GBS * 128, G2_NBUF = 4, G2_NI = GBS / 8 / NLOAD;
static_assert((size_t)G2_NBUF * G2_STAGE <= DmaCfg<GRS>::STAGE_BYTES, "second ring inside the first");
constexpr int G_CUS = 256;        // workgroups that fill the chip
constexpr float HALF_MAX = 60000.f;
constexpr int G_NCH_MAX = 8, G_NCH_MIN = 4;   // the slab widths that are shipped (Makefile: no scratch in either)

struct BwdValuesWs {
    float *mb, *ascale, *rqp, *glsp, *part;
};
struct BwdValuesPlan {
    int n_stiles, n_qtiles, nch, nslabs, nchunks, tpc;
};
struct BwdValuesArgs {
    const float *q, *s, *s_scale, *s_norm2, *v, *v_scale, *gout;
    const int *win_lo, *win_hi;
    const float *lse, *logit_scale, *row_logw;
    BwdValuesWs ws;
    int exclude, B, N, d, T, n_stiles, n_qtiles, nslabs, nchunks, tpc;
};

// m_b = g_b . out_b: one workgroup per query.  (A thread adds its columns in order, the block in a fixed tree: deterministic.)
__global__ __launch_bounds__(256) void nw_bwd_values_prologue_kernel(const float* __restrict__ out, const float* __restrict__ gout,
                                                                      float* __restrict__ mb, int64_t T) {
    __shared__ float red[8];
    const int64_t b = blockIdx.x;
    float t = 0.f;
    for (int64_t c = threadIdx.x; c < T; c += 256) t = __builtin_fmaf(gout[b * T + c], out[b * T + c], t);
    t = block_sum(t, red);
    if (threadIdx.x == 0) mb[b] = t;
}

template <int KIND, int NCH>
__global__ __launch_bounds__(TILE_THREADS, 2) void nw_bwd_values_query_kernel(const BwdValuesArgs a) {
    constexpr bool NEED_NORM = (KIND != NW_SCORE_DOT);
    constexpr float L2E = 1.44269504088896340736f, LN2 = 0.693147180559945309417f;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* qn2 = reinterpret_cast<float*>(smem);
    float* qsc_s = qn2 + BQ;
    float* fac_s = qsc_s + BQ;       // rescaling factors of the rows, wave-private
    float* gn2 = fac_s + BQ;         // the second product's row statistics: |g_b|^2 (not used) ...
    float* gsc_s = gn2 + BQ;         // ... and the gout rows' 2^-e_b
    float* sn2 = gsc_s + BQ;
    float* ssc = sn2 + GBS;
    float* vsc = ssc + GBS;          // the value rows' 2^-e_j
    float* law = vsc + GBS;          // the tile's row log-weights (0 without them: the fused multiply-add is then exact)
    float4* stage = reinterpret_cast<float4*>(smem + G_HDR);
    const char* ring2 = smem + G_HDR;

    const int B = a.B, N = a.N, d = a.d, T = a.T;
    const int tid = threadIdx.x, lane = tid & 63, i = lane & 15, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // workgroup -> (chunk, slab, query tile): the workgroups that share a chunk's bank rows are neighbours
    const int qt = blockIdx.x % a.n_qtiles, rest = blockIdx.x / a.n_qtiles;
    const int slab = rest % a.nslabs, chunk = rest / a.nslabs;
    const int q0 = qt * BQ;
    const int nk = d / BK, nkt = T / BK;
    const int kc0 = slab * NCH;
    const int nc = min(NCH, nk - kc0);                 // 32-column chunks of this slab
    const int st_begin = chunk * a.tpc, st_end = min(a.n_stiles, st_begin + a.tpc);

    // ---- what a consumer lane knows of its query (query 16 wave + i on the lane)
    const int qrow = 16 * (wave & 3) + i;
    const int b = q0 + qrow, bb = b < B ? b : B - 1;
    const float lse = a.lse[bb];
    const float lsev = lse == -INFINITY ? INFINITY : lse * L2E;   // a dead query: W = 2^(u - inf) = 0 in every row
    const float mq = a.ws.mb[bb];
    const bool windowed = a.win_lo != nullptr;
    const bool weighted = a.row_logw != nullptr;
    int lo = 0, hi = N;
    if (windowed) lo = min(max(a.win_lo[bb], 0), N), hi = min(max(a.win_hi[bb], 0), N);   // never used as addresses
    const unsigned width = hi > lo ? (unsigned)(hi - lo) : 0u;
    const bool exclude = a.exclude != 0;

    f32x4 gacc[NCH][2];
#pragma unroll
    for (int c = 0; c < NCH; ++c) gacc[c][0] = gacc[c][1] = f32x4{0.f, 0.f, 0.f, 0.f};
    float rq_acc = 0.f, gls_acc = 0.f;
    int Erun = 0;          // the row's exponent in this chunk so far; `have`: some tile has set it
    bool have = false;

    // transposed reads of the third product (bwd_query.hip): lane 4q + p of group g supplies row 4g + q (+ 16h + 32t),
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
        const int s0 = st * GBS;
        for (int t = tid; t < GBS; t += TILE_THREADS) {
            const int j = min(s0 + t, N - 1);
            if (NEED_NORM) sn2[t] = a.s_norm2[j];
            ssc[t] = a.s_scale[j];
            vsc[t] = a.v_scale[j];
            law[t] = weighted ? a.row_logw[j] : 0.f;
        }
        f32x4 acc[GRS], acc2[GRS];
        tile_dots_f16x2<GRS, true>(a.q, a.s, B, N, d, q0, s0, stage, acc, st % nk, qn2, qsc_s);
        __syncthreads();   // the ring of the first product is dead
        tile_dots_f16x2<GRS, true>(a.gout, a.v, B, N, T, q0, s0, stage, acc2, st % nkt, gn2, gsc_s);
        __syncthreads();   // the header is visible, the ring is dead

        if (wave < NCONS) {
            // ================================ consumers: A' in registers ================================
            half8 Ah[GRS / 2], Al[GRS / 2];
            {
                using SF = ScoreFactors<KIND>;
                const float qn = NEED_NORM ? qn2[qrow] : 0.f;
                const float gs = gsc_s[qrow];
                float scale, nq, inq2, Cq, Bq;
                bwd_query_factors<KIND>(qn, a.logit_scale, scale, nq, inq2);
                SF::query(qn, qsc_s[qrow], scale, Cq, Bq);
                const int tile_end = s0 + GBS < N ? s0 + GBS : N;
                // the window's rule of the forward (fused_impl.h, OUT_WIN): a pair the window leaves whole skips the comparisons
                const bool whole = !windowed || (exclude ? (width == 0u || hi <= s0 || lo >= tile_end) : (lo <= s0 && hi >= tile_end));
                const bool check = !whole || tile_end < s0 + GBS;
                const int rel = s0 + 4 * g - lo;
                float xr[GRS][4], amax = 0.f;
#pragma unroll
                for (int r = 0; r < GRS; ++r) {
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
                        // the weighted score (the forward's fused multiply-add) goes into W alone: bwd_pair_coeff below takes
                        // the raw score, whose distance the kind's derivative is a function of
                        float W = __builtin_amdgcn_exp2f(__builtin_fmaf(aw[e], L2E, u) - lsev);
                        if (check) {
                            const int t = 16 * r + e;
                            bool keep = s0 + 4 * g + t < N;
                            if (windowed) keep = keep && (((unsigned)(rel + t) < width) != exclude);
                            W = keep ? W : 0.f;
                        }
                        const float cv = acc2[r][e] * (gs * vs[e]);   // both scales are powers of two: exact
                        const float dS = W * (cv - mq);
                        float av, rs_unused;
                        bwd_pair_coeff<KIND>(u * LN2, dS, nn[e], scale, nq, inq2, av, rs_unused, rq_acc, gls_acc);
                        xr[r][e] = av * ss[e];
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
                for (int r = 0; r < GRS; ++r)
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
                        gacc[c][0] *= fv;
                        gacc[c][1] *= fv;
                    }
                }
            }
            // ================================ consumers: gq tile += A' s' ================================
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
                    const char* buf = ring2 + (c % G2_NBUF) * G2_STAGE;
#pragma unroll
                    for (int t = 0; t < GRS / 2; ++t) {
                        const half8 bh0 = tr8(buf, toff[0][0] + 32 * 128 * t), bh1 = tr8(buf, toff[0][1] + 32 * 128 * t);
                        const half8 bl0 = tr8(buf, toff[1][0] + 32 * 128 * t), bl1 = tr8(buf, toff[1][1] + 32 * 128 * t);
                        // small terms first, the dominant h*h product last; the two column blocks alternate
                        gacc[c][0] = mm(Al[t], bh0, gacc[c][0]);
                        gacc[c][1] = mm(Al[t], bh1, gacc[c][1]);
                        gacc[c][0] = mm(Ah[t], bl0, gacc[c][0]);
                        gacc[c][1] = mm(Ah[t], bl1, gacc[c][1]);
                        gacc[c][0] = mm(Ah[t], bh0, gacc[c][0]);
                        gacc[c][1] = mm(Ah[t], bh1, gacc[c][1]);
                    }
                }
            }
            tile_barrier();   // the ring is free for the next tile
        } else {
            // ================================ loaders: the tile's bank rows again, this slab's columns ================================
            const int lw = wave - NCONS;
            unsigned voff[G2_NI];
#pragma unroll
            for (int m = 0; m < G2_NI; ++m) {
                const int R = 8 * (lw + NLOAD * m) + (lane >> 3);
                const int lslot = (lane & 7) ^ (((R >> 1) & 3) << 1);   // source-side swizzle (see toff)
                const int rel = min(s0 + R, N - 1) - s0;                // a row past N repeats row N - 1: its coefficient is 0
                voff[m] = ((unsigned)rel * (unsigned)d + lslot * 4) * 4u;
            }
            const char* sb = reinterpret_cast<const char*>(a.s + (size_t)s0 * d) + (size_t)kc0 * BK * 4;
            auto issue = [&](int c) {
                char* buf = smem + G_HDR + (c % G2_NBUF) * G2_STAGE;
#pragma unroll
                for (int m = 0; m < G2_NI; ++m)
                    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(sb + (size_t)c * BK * 4 + voff[m]),
                                                     (__attribute__((address_space(3))) void*)(buf + 1024 * (lw + NLOAD * m)), 16, 0, 0);
            };
            constexpr int AHEAD = G2_NBUF - 1;
#pragma unroll
            for (int c = 0; c < AHEAD; ++c)
                if (c < nc) issue(c);
            for (int c = 0; c < nc; ++c) {
                if (c + AHEAD <= nc) wait_vmcnt<(AHEAD - 1) * G2_NI>(); else wait_vmcnt<0>();
                tile_barrier();   // stage c is published; the consumers have left stage c - 1
                if (c + AHEAD < nc) issue(c + AHEAD);
            }
            tile_barrier();
        }
    }

    if (wave >= NCONS) return;
    // ---- partial results of this chunk: gacc[c][nb][e] of lane (i, g) = gq'[query 16 wave + 4g + e][column 32 (kc0 + c) + 16 nb + i]
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        if (c < nc) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int bo = q0 + 16 * wave + 4 * g + e;
                if (bo < B) {
                    float* row = a.ws.part + ((size_t)chunk * B + bo) * d + (size_t)(kc0 + c) * BK + i;
                    row[0] = gacc[c][0][e];
                    row[16] = gacc[c][1][e];
                }
            }
        }
    }
    if (slab == 0) {
        rq_acc = group4_sum(rq_acc);
        gls_acc = group4_sum(gls_acc);
        if (g == 0 && b < B) {
            a.ws.rqp[(size_t)chunk * B + b] = rq_acc;
            a.ws.glsp[(size_t)chunk * B + b] = gls_acc;
            a.ws.ascale[(size_t)chunk * B + b] = __builtin_ldexpf(1.f, -Erun);   // (1 when no tile set it: the partial row is zero)
        }
    }
}

// gq[b,k] = sum_chunks 2^-E[c][b] part[c][b,k] + 2 (sum_chunks rq[c][b]) q[b,k], chunks in order (k in float4s).  (The
// query gradient's finish kernels live in bwd_query.hip's unnamed namespace, a file this one leaves alone: copies.)
__global__ __launch_bounds__(256) void nw_bwd_values_finish_kernel(const float* __restrict__ part, const float* __restrict__ rqp,
                                                                    const float* __restrict__ ascale, const float* __restrict__ q,
                                                                    float* __restrict__ gq, int nchunks, int64_t B, int64_t d) {
    const int64_t total4 = B * d / 4;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total4) return;
    const int64_t b = (idx * 4) / d;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    float rq = 0.f;
    for (int c = 0; c < nchunks; ++c) {
        const float4 w = *reinterpret_cast<const float4*>(part + (int64_t)c * B * d + idx * 4);
        const float f = ascale[(int64_t)c * B + b];   // a power of two: exact
        v.x += w.x * f; v.y += w.y * f; v.z += w.z * f; v.w += w.w * f;
        rq += rqp[(int64_t)c * B + b];
    }
    const float r2 = 2.f * rq;
    const float4 x = *reinterpret_cast<const float4*>(q + idx * 4);
    v.x = __builtin_fmaf(r2, x.x, v.x); v.y = __builtin_fmaf(r2, x.y, v.y);
    v.z = __builtin_fmaf(r2, x.z, v.z); v.w = __builtin_fmaf(r2, x.w, v.w);
    *reinterpret_cast<float4*>(gq + idx * 4) = v;
}

// glogit_scale = sum_b sum_chunks gls[c][b]: a thread adds its queries' chunks in order, the block in a fixed tree
__global__ __launch_bounds__(256) void nw_bwd_values_gls_kernel(const float* __restrict__ glsp, float* __restrict__ out, int nchunks,
                                                                 int64_t B) {
    __shared__ float red[8];
    float v = 0.f;
    for (int64_t b = threadIdx.x; b < B; b += 256)
        for (int c = 0; c < nchunks; ++c) v += glsp[(int64_t)c * B + b];
    v = block_sum(v, red);
    if (threadIdx.x == 0) *out = v;
}

// Slab width and chunk count, by bwd_query_plan's model with the extra product: per support tile a workgroup costs
// 3 d/32 for the scores + 3 T/32 for c (every slab recomputes both) + 4 per 32 columns of its slab; the grid runs in
// ceil(workgroups / CUs) rounds.  The workspace cap is the query gradient's: the library's own choice keeps the partial
// tiles, nchunks B d 4 bytes, below 0.85 B N bytes.
BwdValuesPlan bwd_values_plan(int64_t B, int64_t N, int64_t d, int64_t T, int row_chunks) {
    BwdValuesPlan best = {};
    const int64_t n_stiles = (N + GBS - 1) / GBS, n_qtiles = (B + BQ - 1) / BQ, nk = d / BK, nkt = T / BK;
    int64_t best_cost = -1;
    for (int nch = G_NCH_MAX; nch >= G_NCH_MIN; nch >>= 1) {
        if (nch > G_NCH_MIN && nch / 2 >= nk) continue;   // a narrower slab already takes the whole width
        const int64_t nslabs = (nk + nch - 1) / nch;
        int64_t want;
        if (row_chunks > 0) {
            want = row_chunks < n_stiles ? row_chunks : n_stiles;
        } else {
            const int64_t fit = n_stiles * GBS * 27 / (128 * d), cap = fit > 1 ? fit : 1;
            want = (G_CUS + n_qtiles * nslabs - 1) / (n_qtiles * nslabs);
            if (want > cap) want = cap;
        }
        const int64_t tpc = (n_stiles + want - 1) / want, nchunks = (n_stiles + tpc - 1) / tpc;
        const int64_t wgs = n_qtiles * nslabs * nchunks, rounds = (wgs + G_CUS - 1) / G_CUS;
        const int64_t cost = rounds * tpc * (3 * nk + 3 * nkt + 4 * (nch < nk ? nch : nk));
        if (best_cost < 0 || cost < best_cost) {
            best_cost = cost;
            best = {(int)n_stiles, (int)n_qtiles, nch, (int)nslabs, (int)nchunks, (int)tpc};
        }
    }
    return best;
}

// mb | ascale | rqp | glsp | part
size_t bwd_values_layout(int64_t B, int64_t d, const BwdValuesPlan& p, char* base, BwdValuesWs* ws) {
    size_t off = 0;
    auto take = [&](size_t nfloat) {
        float* ptr = base ? reinterpret_cast<float*>(base + off) : nullptr;
        off += align256(nfloat * sizeof(float));
        return ptr;
    };
    BwdValuesWs w;
    w.mb = take((size_t)B);
    w.ascale = take((size_t)p.nchunks * B);
    w.rqp = take((size_t)p.nchunks * B);
    w.glsp = take((size_t)p.nchunks * B);
    w.part = take((size_t)p.nchunks * B * d);
    if (ws) *ws = w;
    return off;
}

template <int KIND, int NCH>
int launch_bwd_values_kernel(const BwdValuesArgs& a, unsigned grid, hipStream_t st) {
    static const bool attr = hipFuncSetAttribute(reinterpret_cast<const void*>(nw_bwd_values_query_kernel<KIND, NCH>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)G_LDS) == hipSuccess;
    if (!attr) return NW_ERR_LAUNCH;
    hipLaunchKernelGGL((nw_bwd_values_query_kernel<KIND, NCH>), dim3(grid), dim3(TILE_THREADS), G_LDS, st, a);
    return NW_OK;
}
template <int KIND>
int launch_bwd_values_kind(const BwdValuesArgs& a, int nch, unsigned grid, hipStream_t st) {
    if constexpr (G_NCH_MAX != G_NCH_MIN)
        if (nch == G_NCH_MAX) return launch_bwd_values_kernel<KIND, G_NCH_MAX>(a, grid, st);
    return launch_bwd_values_kernel<KIND, G_NCH_MIN>(a, grid, st);
}

}  // namespace

bool bwd_values_shape_ok(int64_t B, int64_t N, int64_t d, int64_t T) { return fwd_values_shape_ok(B, N, d, T); }

size_t bwd_values_workspace_bytes(int64_t B, int64_t N, int64_t d, int64_t T, int row_chunks) {
    if (B <= 0 || !bwd_values_shape_ok(B, N, d, T)) return 0;
    return bwd_values_layout(B, d, bwd_values_plan(B, N, d, T, row_chunks), nullptr, nullptr);
}

int launch_bwd_values(const BwdValuesCall& c) {
    hipStream_t st = c.st;
    const BwdValuesPlan p = bwd_values_plan(c.B, c.N, c.d, c.T, c.row_chunks);
    BwdValuesWs ws;
    const size_t need = bwd_values_layout(c.B, c.d, p, static_cast<char*>(c.workspace), &ws);
    if (!c.workspace || c.workspace_bytes < need) return NW_ERR_WORKSPACE;
    const int64_t wgs = (int64_t)p.n_qtiles * p.nslabs * p.nchunks;
    if (wgs > 0x7fffffffLL || (c.B * c.d / 4 + 255) / 256 > 0x7fffffffLL) return NW_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(nw_bwd_values_prologue_kernel, dim3((unsigned)c.B), dim3(256), 0, st, c.out, c.gout, ws.mb, c.T);
    const BwdValuesArgs a = {c.q, c.s_split, c.s_scale, c.s_norm2, c.v_split, c.v_scale, c.gout, c.row_lo, c.row_hi, c.lse,
                             c.logit_scale_dev, c.row_logw, ws, c.row_lo && c.exclude != 0, (int)c.B, (int)c.N, (int)c.d, (int)c.T,
                             p.n_stiles, p.n_qtiles, p.nslabs, p.nchunks, p.tpc};
    int rc;
    switch (c.kind) {
        case NW_SCORE_EUCLIDEAN: rc = launch_bwd_values_kind<NW_SCORE_EUCLIDEAN>(a, p.nch, (unsigned)wgs, st); break;
        case NW_SCORE_HYPERSPHERE: rc = launch_bwd_values_kind<NW_SCORE_HYPERSPHERE>(a, p.nch, (unsigned)wgs, st); break;
        case NW_SCORE_COSINE: rc = launch_bwd_values_kind<NW_SCORE_COSINE>(a, p.nch, (unsigned)wgs, st); break;
        case NW_SCORE_DOT: rc = launch_bwd_values_kind<NW_SCORE_DOT>(a, p.nch, (unsigned)wgs, st); break;
        default: rc = launch_bwd_values_kind<NW_SCORE_CLIP>(a, p.nch, (unsigned)wgs, st); break;
    }
    if (rc != NW_OK) return rc;
    hipLaunchKernelGGL(nw_bwd_values_finish_kernel, dim3((unsigned)((c.B * c.d / 4 + 255) / 256)), dim3(256), 0, st, ws.part, ws.rqp,
                       ws.ascale, c.q, c.gq, p.nchunks, c.B, c.d);
    if (c.glogit_scale) {
        if (c.kind == NW_SCORE_CLIP)
            hipLaunchKernelGGL(nw_bwd_values_gls_kernel, dim3(1), dim3(256), 0, st, ws.glsp, c.glogit_scale, p.nchunks, c.B);
        else if (hipMemsetAsync(c.glogit_scale, 0, 4, st) != hipSuccess)
            return NW_ERR_LAUNCH;
    }
    NW_CHECK_LAUNCH();
    return NW_OK;
}

}  // namespace nw
