// bwd_query.hip -- gradient of the head w.r.t. the queries over a resident split bank, without a (B,N) matrix
// (gfx950 / MI355X only; nw_bwd_query_f32, nw_bwd_query_weighted_f32), and w.r.t. the row weights (nw_bwd_query_logw_f32).
//
// backward.hip's closed form with the bank a constant.  For query b, bank row j, score s_bj = f(dot, |q_b|^2, |s_j|^2):
//     dP_c = g_bc exp(-out_bc)                 dW_j = dP[y_j]  (0 for a label outside [0, C))
//     W_j  = exp(s_bj - lse_b) for a row the window admits, 0 otherwise
//            (row weights, WGT: exp(s_bj + a_j - lse_b), lse and out those of the weighted forward.  The weights are a
//            constant: only W carries a_j, the derivatives df/d. below are taken at the raw score s_bj)
//     t_b  = sum_j W_j dW_j                    dS_j = W_j (dW_j - t_b)
//     A_bj = dS_j df/ddot     rq_b = sum_j dS_j df/d|q|^2     gls = sum_bj dS_j df/dlogit_scale   (bwd_coeff.h)
//     gq_b = sum_j A_bj s_j + 2 rq_b q_b
// Nothing of size B x N is read or written: a workgroup owns 64 queries, a contiguous chunk of 64-row support tiles and a
// slab of 32 * NCH columns of d.  Per support tile it
//   1. recomputes the tile's dot products like the forward does (tile_dots_f16x2: raw queries split in registers, split
//      bank rows, LDS-DMA ring) -- query on the lane, support rows 16r + 4g + e in the registers;
//   2. turns them into A in registers (score, window, W, dW gathered from the (B,C) table of the prologue, dS, the kind's
//      derivative), scales the row by 2^E_b and the element by the bank row's 2^-e_j, and splits it into fp16 halves;
//   3. streams the tile's bank rows once more, 32 columns at a time, and adds A' s' to its 64 x (32 NCH) accumulators on
//      v_mfma_f32_16x16x32_f16 (hl, lh, hh).  The accumulator layout of step 1 IS the A-operand layout of this product
//      (query = row, eight supports per lane = k), with the k order permuted: element e of block r is tile row
//      16r + 4g + e.  The bank operand is read with ds_read_b64_tr_b16 in the same order: lane 4q + p of group g supplies
//      row 32t + 16h + 4g + q, columns 4p .. 4p + 3 of the 16-column block.
// t_b needs no pass over the bank: it is sum_c dP_c P_c with P_c = exp(out_c) - 1e-12 the class mass.  A class that no
// admitted row carries has out_c = log(1e-12) exactly (the forward adds 1e-12 to an exact 0) and is left out, so that it
// contributes exactly 0 (the closed form through the rounded `out` would give ~1e-6 g).
//
// Scaling.  s'_j = s_j 2^e_j are the bank's rows; A'_bj = A_bj 2^-e_j 2^E with ONE exponent per query row and chunk, a
// power of two: gq_b = sum_chunks 2^-E_{b,chunk} sum_j A'_bj s'_j + 2 rq_b q_b, and scaling a row of gout by 2^k scales its
// row of gq exactly.  E is known before a tile is multiplied, without a pass over the row: it is the split exponent of the
// largest |A_bj 2^-e_j| the row has shown SO FAR in the chunk (taken in registers, per tile), and when a tile raises it
// the row's accumulators are rescaled by the power of two between the old and the new exponent (exact; the factor
// crosses from "query on the lane" to "query in the registers" through 64 floats of LDS that a wave writes and reads
// itself).  An a-priori bound does not do for the distance kinds: |df/ddot| = 1/D has none, and the bounds that hold
// (D >= -lse, or the rounding noise of D where lse >= 0) lie 2^12 above the row's real maximum for a large bank
// (lse ~ ln N - D), which costs the small coefficients their low halves: measured 1.5e-3 of max|gq| at 64 x 65536 x 64
// against 1e-4 for the route through the matrix.  An element keeps 22 bits down to 2^-28 of the running maximum.
//
// Chunks over N fill the chip; each writes its partial gq / rq / gls, nw_bwd_query_finish_kernel adds them in chunk order:
// no float atomics, two calls give the same bits.
//
// The gradient w.r.t. the row weights (GA; nw_bwd_query_logw_f32).  d out / d a_j is the column sum of the dS above,
//     ga_j = sum_b dS_bj,
// taken from the registers that hold dS for the row contraction: a consumer lane (i, g) of wave w holds dS for query
// 16w + i and the 16 tile rows 16r + 4g + e.  Per support tile
//   1. the 16 lanes i of a lane group reduce-scatter their 16 values in 15 DPP exchanges (partners i ^ 8, i ^ 7, i ^ 2,
//      i ^ 1; a lane sends the half it does not keep): lane i ends with the sum over the wave's 16 queries of row
//      16 (i >> 2) + 4g + (i & 3);
//   2. the four consumer waves write their 64 sums to a 64 rows x 4 waves float area beside the header; behind the next
//      workgroup barrier the first loader wave adds the four in wave order and stores the tile's 64 sums to
//      gap[query tile][row].  With gq (GA = 1) that barrier is the first of the second product, which every wave passes
//      anyway; without (GA = 2) it is the tile's only barrier behind the scores.
// Only slab 0 writes (every slab recomputes the same scores); chunks own disjoint rows, so the chunk count does not enter
// the sum; nw_bwd_logw_finish_kernel adds the query tiles in ascending order from +0: no float atomics, a row that nobody
// admits is +0.0 exactly.  GA = 2 (gq == NULL, a frozen featurizer) drops the second stream of the bank rows, the second
// product and the part / rqp / ascale areas; its dS and its reduction are GA = 1's, so ga is the same bit for bit.
#include "nw_internal.h"
#include "tile_dma.h"
#include "tile_f16.h"
#include "bwd_coeff.h"

namespace nw {
namespace {

typedef __fp16 fp16x4 __attribute__((__vector_size__(4 * sizeof(__fp16))));
typedef _Float16 halfx4 __attribute__((ext_vector_type(4)));

constexpr int QRS = 4;            // support blocks per tile
constexpr int QBS = 16 * QRS;     // 64 bank rows per tile
constexpr int Q_HDR = (3 * BQ + 3 * QBS) * 4;   // qn2[BQ] | qsc[BQ] | fac[BQ] | sn2[QBS] | ssc[QBS] | lab[QBS]
constexpr int Q_HDR_W = Q_HDR + QBS * 4;        // ... | law[QBS]: the tile's row log-weights (the weighted kernels only)
constexpr int Q_HDR_GA = Q_HDR_W + QBS * NCONS * 4;   // ... | gar[QBS][NCONS]: the waves' column sums of dS (the GA kernels only)
static_assert(Q_HDR % 16 == 0 && Q_HDR_W % 16 == 0 && Q_HDR_GA % 16 == 0, "stage buffers must stay 16-byte aligned");
constexpr size_t Q_LDS = Q_HDR + DmaCfg<QRS>::STAGE_BYTES, Q_LDS_W = Q_HDR_W + DmaCfg<QRS>::STAGE_BYTES;
constexpr size_t Q_LDS_GA = Q_HDR_GA + DmaCfg<QRS>::STAGE_BYTES;
static_assert(Q_LDS_GA <= 80 * 1024, "header + ring exceed the LDS of two workgroups per CU");
// the second product's ring (over the forward's, dead by then): 64 rows x 128 B per stage
constexpr int Q2_STAGE = QBS * 128, Q2_NBUF = 4, Q2_NI = QBS / 8 / NLOAD;
static_assert((size_t)Q2_NBUF * Q2_STAGE <= DmaCfg<QRS>::STAGE_BYTES, "second ring inside the first");
constexpr int Q_CUS = 256;        // workgroups that fill the chip (one per CU: up to 217 registers per lane)
constexpr float HALF_MAX = 60000.f;

struct BwdQueryWs {
    float *dptab, *tb, *ascale, *rqp, *glsp, *part;
};
struct BwdQueryPlan {
    int n_stiles, n_qtiles, nch, nslabs, nchunks, tpc;
};
struct BwdQueryArgs {
    const float *q, *s, *s_scale, *s_norm2;
    const int64_t* sy;
    const int *win_lo, *win_hi;
    const float *lse, *logit_scale, *row_logw;
    BwdQueryWs ws;
    int exclude, B, N, d, C, n_stiles, n_qtiles, nslabs, nchunks, tpc;
    // (behind everything the kernels without GA read, whose argument offsets stay what they were)
    float* gap;   // (n_qtiles, 64 n_stiles) column sums of dS per query tile, the GA kernels only
};

// dP (B,C) and t_b: one workgroup per query.  (The block sum runs in a fixed order: deterministic.)
__global__ __launch_bounds__(256) void nw_bwd_query_prologue_kernel(const float* __restrict__ out, const float* __restrict__ gout,
                                                                     float* __restrict__ dptab, float* __restrict__ tb, int64_t C) {
    __shared__ float red[8];
    const int64_t b = blockIdx.x;
    // what the forward's logf gives for an empty class, from the same routine (blockIdx.y is 0: not folded on the host)
    const float absent = logf((float)blockIdx.y + NW_LOG_EPS);
    float t = 0.f;
    for (int64_t c = threadIdx.x; c < C; c += 256) {
        const float o = out[b * C + c];
        float dp = 0.f;
        if (o > absent) {
            dp = gout[b * C + c] * expf(-o);
            t += dp * (expf(o) - NW_LOG_EPS);
        }
        dptab[b * C + c] = dp;
    }
    t = block_sum(t, red);
    if (threadIdx.x == 0) tb[b] = t;
}

// One step of the reduce-scatter over the 16 lanes of a lane group: partner = the lane a DPP control CTL pairs this one
// with (an involution that flips the lane bit `upper` is read from); a lane keeps the half of its 2 H values that its
// bit selects, adds the partner's values of that half, and sends the other half.  Plain additions, never contracted with
// the product that made an operand: GA = 1 and GA = 2 must round alike.
template <int CTL, int H>
__device__ __forceinline__ void colsum_step(const float (&in)[2 * H], float (&outv)[H], bool upper) {
#pragma clang fp contract(off)
#pragma unroll
    for (int k = 0; k < H; ++k) {
        const float keep = upper ? in[H + k] : in[k], send = upper ? in[k] : in[H + k];
        outv[k] = keep + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, send), CTL, 0xf, 0xf, false));
    }
}
// v[4r + e] = dS of the lane's query for tile row 16r + 4g + e -> the sum over the 16 lanes i of the group of value i,
// i.e. of tile row 16 (i >> 2) + 4g + (i & 3)
__device__ __forceinline__ float colsum16(const float (&v)[16], int i) {
    float v8[8], v4[4], v2[2], v1[1];
    colsum_step<0x128, 8>(v, v8, (i & 8) != 0);    // row_ror:8            i ^ 8
    colsum_step<0x141, 4>(v8, v4, (i & 4) != 0);   // row_half_mirror      i ^ 7
    colsum_step<0x4e, 2>(v4, v2, (i & 2) != 0);    // quad_perm [2,3,0,1]  i ^ 2
    colsum_step<0xb1, 1>(v2, v1, (i & 1) != 0);    // quad_perm [1,0,3,2]  i ^ 1
    return v1[0];
}

// WGT: a.row_logw holds a natural-log weight per bank row, staged per tile beside the labels (a fourth header array).
// GA (WGT only): 0 -- gq alone; 1 -- gq and the weights' gradient; 2 -- the weights' gradient alone (no second product:
// NCH is 1 and names nothing, one slab).  See the header.
template <int KIND, int NCH, bool WGT, int GA = 0>
__global__ __launch_bounds__(TILE_THREADS, 2) void nw_bwd_query_kernel(const BwdQueryArgs a) {
    static_assert(GA == 0 || WGT, "the weights' gradient belongs to the weighted head");
    static_assert(GA != 2 || NCH == 1, "the weights-only kernel has no slab");
    constexpr bool NEED_NORM = (KIND != NW_SCORE_DOT);
    constexpr bool GQ = GA != 2;
    constexpr int HDR = GA ? Q_HDR_GA : (WGT ? Q_HDR_W : Q_HDR);
    constexpr float L2E = 1.44269504088896340736f, LN2 = 0.693147180559945309417f;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* qn2 = reinterpret_cast<float*>(smem);
    float* qsc_s = qn2 + BQ;
    float* fac_s = qsc_s + BQ;       // rescaling factors of the rows, wave-private (see the header)
    float* sn2 = fac_s + BQ;
    float* ssc = sn2 + QBS;
    int* lab = reinterpret_cast<int*>(ssc + QBS);
    float* law = reinterpret_cast<float*>(lab + QBS);   // (WGT only)
    float* gar = law + QBS;                             // (GA only) [tile row][consumer wave]
    float4* stage = reinterpret_cast<float4*>(smem + HDR);
    const char* ring2 = smem + HDR;

    const int B = a.B, N = a.N, d = a.d;
    const int tid = threadIdx.x, lane = tid & 63, i = lane & 15, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // workgroup -> (chunk, slab, query tile): the workgroups that share a chunk's bank rows are neighbours
    const int qt = blockIdx.x % a.n_qtiles, rest = blockIdx.x / a.n_qtiles;
    const int slab = rest % a.nslabs, chunk = rest / a.nslabs;
    const int q0 = qt * BQ;
    const int nk = d / BK;
    const int kc0 = slab * NCH;
    const int nc = min(NCH, nk - kc0);                 // 32-column chunks of this slab
    const int st_begin = chunk * a.tpc, st_end = min(a.n_stiles, st_begin + a.tpc);
    // the tile's 64 column sums, by the first loader wave behind the barrier that follows the consumers' writes of `gar`
    auto store_colsums = [&](int s0) {
        const float4 v = *reinterpret_cast<const float4*>(gar + NCONS * lane);
        a.gap[(size_t)qt * ((size_t)a.n_stiles * QBS) + s0 + lane] = ((v.x + v.y) + v.z) + v.w;
    };

    // ---- what a consumer lane knows of its query (query 16 wave + i on the lane)
    const int qrow = 16 * (wave & 3) + i;
    const int b = q0 + qrow, bb = b < B ? b : B - 1;
    const float lse = a.lse[bb];
    const float lsev = lse == -INFINITY ? INFINITY : lse * L2E;   // a dead window: W = 2^(u - inf) = 0 in every row
    const float tq = a.ws.tb[bb];
    const float* dprow = a.ws.dptab + (size_t)bb * a.C;
    const bool windowed = a.win_lo != nullptr;
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

    // transposed reads of the second product: lane 4q + p of group g supplies row 4g + q (+ 16h + 32t), bytes 8(p & 1) of
    // 16-byte slot (gs + (p >> 1)) ^ sw, sw = 2 ((row >> 1) & 3): the eight rows a 32-lane half touches land on eight
    // different groups of eight banks
    const int tq4 = i >> 2, tp = i & 3;
    const int sw2 = ((2 * g + (tq4 >> 1)) & 3) << 1;
    const int trow = (4 * g + tq4) * 128 + 8 * (tp & 1);
    int toff[2][2];   // [half: h, l][16-column block]
#pragma unroll
    for (int hl = 0; hl < 2; ++hl)
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) toff[hl][nb] = trow + (((4 * hl + 2 * nb + (tp >> 1)) ^ sw2) << 4);

    for (int st = st_begin; st < st_end; ++st) {
        const int s0 = st * QBS;
        for (int t = tid; t < QBS; t += TILE_THREADS) {
            const int j = min(s0 + t, N - 1);
            if (NEED_NORM) sn2[t] = a.s_norm2[j];
            ssc[t] = a.s_scale[j];
            const int64_t y = a.sy[j];
            lab[t] = ((uint64_t)y < (uint64_t)a.C) ? (int)y : -1;
            if constexpr (WGT) law[t] = a.row_logw[j];
        }
        f32x4 acc[QRS];
        tile_dots_f16x2<QRS, true>(a.q, a.s, B, N, d, q0, s0, stage, acc, st % nk, qn2, qsc_s);
        __syncthreads();   // the header is visible, the ring is dead

        if (wave < NCONS) {
            // ================================ consumers: A' in registers ================================
            half8 Ah[QRS / 2], Al[QRS / 2];
            {
                using SF = ScoreFactors<KIND>;
                const float qn = NEED_NORM ? qn2[qrow] : 0.f;
                float scale, nq, inq2, Cq, Bq;
                bwd_query_factors<KIND>(qn, a.logit_scale, scale, nq, inq2);
                SF::query(qn, qsc_s[qrow], scale, Cq, Bq);
                const int tile_end = s0 + QBS < N ? s0 + QBS : N;
                // the window's rule of the forward (fused_impl.h, OUT_WIN): a pair the window leaves whole skips the comparisons
                const bool whole = !windowed || (exclude ? (width == 0u || hi <= s0 || lo >= tile_end) : (lo <= s0 && hi >= tile_end));
                const bool check = !whole || tile_end < s0 + QBS;
                const int rel = s0 + 4 * g - lo;
                float dw[QRS][4], xr[QRS][4], amax = 0.f;
                float dsv[GA ? 4 * QRS : 1];   // (GA) the lane's dS, for the column sums
#pragma unroll
                for (int r = 0; r < QRS; ++r) {
                    const int4 y4 = *reinterpret_cast<const int4*>(lab + 16 * r + 4 * g);
                    const int yy[4] = {y4.x, y4.y, y4.z, y4.w};
#pragma unroll
                    for (int e = 0; e < 4; ++e) dw[r][e] = dprow[yy[e] < 0 ? 0 : yy[e]];
#pragma unroll
                    for (int e = 0; e < 4; ++e) dw[r][e] = yy[e] < 0 ? 0.f : dw[r][e];
                }
#pragma unroll
                for (int r = 0; r < QRS; ++r) {
                    float4 n4 = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (NEED_NORM) n4 = *reinterpret_cast<const float4*>(sn2 + 16 * r + 4 * g);
                    const float4 s4 = *reinterpret_cast<const float4*>(ssc + 16 * r + 4 * g);
                    const float nn[4] = {n4.x, n4.y, n4.z, n4.w}, ss[4] = {s4.x, s4.y, s4.z, s4.w};
                    float4 a4 = make_float4(0.f, 0.f, 0.f, 0.f);
                    if constexpr (WGT) a4 = *reinterpret_cast<const float4*>(law + 16 * r + 4 * g);
                    const float aw[4] = {a4.x, a4.y, a4.z, a4.w};
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        float K, Base;
                        SF::support(nn[e], ss[e], K, Base);
                        const float u = SF::finish(__builtin_fmaf(acc[r][e], K * Cq, Base + Bq));   // base-2 units, as the forward
                        // the weighted score (the forward's fused multiply-add) goes into W alone: bwd_pair_coeff below takes
                        // the raw score, whose distance the kind's derivative is a function of
                        float W = __builtin_amdgcn_exp2f((WGT ? __builtin_fmaf(aw[e], L2E, u) : u) - lsev);
                        if (check) {
                            const int t = 16 * r + e;
                            bool keep = s0 + 4 * g + t < N;
                            if (windowed) keep = keep && (((unsigned)(rel + t) < width) != exclude);
                            W = keep ? W : 0.f;
                        }
                        const float dS = W * (dw[r][e] - tq);
                        if constexpr (GA != 0) dsv[4 * r + e] = b < B ? dS : 0.f;   // (a lane past B repeats query B - 1)
                        float av, rs_unused;
                        bwd_pair_coeff<KIND>(u * LN2, dS, nn[e], scale, nq, inq2, av, rs_unused, rq_acc, gls_acc);
                        xr[r][e] = av * ss[e];
                        amax = fmaxf(amax, fabsf(xr[r][e]));
                    }
                }
                if constexpr (GA != 0) {
                    // the column sums of dS over this wave's 16 queries -> gar[tile row][wave] (only slab 0 writes them out)
                    if (GA == 2 || slab == 0) gar[NCONS * (16 * (i >> 2) + 4 * g + (i & 3)) + wave] = colsum16(dsv, i);
                }
                if constexpr (GQ) {
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
                for (int r = 0; r < QRS; ++r)
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
                }   // GQ
            }
            if constexpr (!GQ) {
                tile_barrier();   // gar is whole; (behind it the first loader wave reads it, the next tile's header may be written)
            } else {
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
                    const char* buf = ring2 + (c % Q2_NBUF) * Q2_STAGE;
#pragma unroll
                    for (int t = 0; t < QRS / 2; ++t) {
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
            }   // GQ
        } else if constexpr (!GQ) {
            // ================================ loaders, weights only: nothing to stream; the tile's column sums ================================
            tile_barrier();
            if (wave == NCONS) store_colsums(s0);
        } else {
            // ================================ loaders: the tile's rows again, this slab's columns ================================
            const int lw = wave - NCONS;
            unsigned voff[Q2_NI];
#pragma unroll
            for (int m = 0; m < Q2_NI; ++m) {
                const int R = 8 * (lw + NLOAD * m) + (lane >> 3);
                const int lslot = (lane & 7) ^ (((R >> 1) & 3) << 1);   // source-side swizzle (see toff)
                const int rel = min(s0 + R, N - 1) - s0;
                voff[m] = ((unsigned)rel * (unsigned)d + lslot * 4) * 4u;
            }
            const char* sb = reinterpret_cast<const char*>(a.s + (size_t)s0 * d) + (size_t)kc0 * BK * 4;
            auto issue = [&](int c) {
                char* buf = smem + HDR + (c % Q2_NBUF) * Q2_STAGE;
#pragma unroll
                for (int m = 0; m < Q2_NI; ++m)
                    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(sb + (size_t)c * BK * 4 + voff[m]),
                                                     (__attribute__((address_space(3))) void*)(buf + 1024 * (lw + NLOAD * m)), 16, 0, 0);
            };
            constexpr int AHEAD = Q2_NBUF - 1;
#pragma unroll
            for (int c = 0; c < AHEAD; ++c)
                if (c < nc) issue(c);
            for (int c = 0; c < nc; ++c) {
                if (c + AHEAD <= nc) wait_vmcnt<(AHEAD - 1) * Q2_NI>(); else wait_vmcnt<0>();
                tile_barrier();   // stage c is published; the consumers have left stage c - 1
                if constexpr (GA == 1) {
                    // (gar was written in front of this product's first barrier.  The store is one more vector-memory
                    // operation in flight: the counted waits above then wait for one more of the older loads, never fewer)
                    if (c == 0 && slab == 0 && lw == 0) store_colsums(s0);
                }
                if (c + AHEAD < nc) issue(c + AHEAD);
            }
            tile_barrier();
        }
    }

    if (wave >= NCONS) return;
    if constexpr (!GQ) {   // the weights alone: of the chunk's partial results only the logit scale's
        gls_acc = group4_sum(gls_acc);
        if (g == 0 && b < B) a.ws.glsp[(size_t)chunk * B + b] = gls_acc;
        return;
    }
    // ---- partial results of this chunk: acc[c][nb][e] of lane (i, g) = gq'[query 16 wave + 4g + e][column 32 (kc0 + c) + 16 nb + i]
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

// gq[b,k] = sum_chunks 2^-E[c][b] part[c][b,k] + 2 (sum_chunks rq[c][b]) q[b,k], chunks in order (k in float4s)
__global__ __launch_bounds__(256) void nw_bwd_query_finish_kernel(const float* __restrict__ part, const float* __restrict__ rqp,
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
__global__ __launch_bounds__(256) void nw_bwd_query_gls_kernel(const float* __restrict__ glsp, float* __restrict__ out, int nchunks,
                                                                int64_t B) {
    __shared__ float red[8];
    float v = 0.f;
    for (int64_t b = threadIdx.x; b < B; b += 256)
        for (int c = 0; c < nchunks; ++c) v += glsp[(int64_t)c * B + b];
    v = block_sum(v, red);
    if (threadIdx.x == 0) *out = v;
}

// ga[j] = sum_qt gap[qt][j], query tiles in ascending order, from +0: a row whose every term is -0 (W = 0 times a
// negative dW - t) comes out +0.0
__global__ __launch_bounds__(256) void nw_bwd_logw_finish_kernel(const float* __restrict__ gap, float* __restrict__ ga, int n_qtiles,
                                                                  int64_t stride, int64_t N) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= N) return;
    float v = 0.f;
    for (int qt = 0; qt < n_qtiles; ++qt) v += gap[(int64_t)qt * stride + j];
    ga[j] = v;
}

// Slab width and chunk count.  Cost of a workgroup per support tile, in matrix-core time: 3 d/32 for the scores (every
// slab recomputes them) + 4 per 32 columns of the slab (3 MFMAs per block and the transposed reads, which bound it);
// the grid runs in ceil(workgroups / CUs) rounds.  The partial tiles are what the workspace holds: the library's own
// choice keeps nchunks B d 4 bytes below 0.85 B N bytes (a fifth of one score matrix), i.e. a chunk is at least d / 27 tiles.
BwdQueryPlan bwd_query_plan(int64_t B, int64_t N, int64_t d, int row_chunks) {
    BwdQueryPlan best = {};
    const int64_t n_stiles = (N + QBS - 1) / QBS, n_qtiles = (B + BQ - 1) / BQ, nk = d / BK;
    int64_t best_cost = -1;
    for (int nch = 8; nch >= 4; nch >>= 1) {
        if (nch > 4 && nch / 2 >= nk) continue;   // a narrower slab already takes the whole width
        const int64_t nslabs = (nk + nch - 1) / nch;
        int64_t want;
        if (row_chunks > 0) {
            want = row_chunks < n_stiles ? row_chunks : n_stiles;
        } else {
            const int64_t fit = n_stiles * QBS * 27 / (128 * d), cap = fit > 1 ? fit : 1;
            want = (Q_CUS + n_qtiles * nslabs - 1) / (n_qtiles * nslabs);
            if (want > cap) want = cap;
        }
        const int64_t tpc = (n_stiles + want - 1) / want, nchunks = (n_stiles + tpc - 1) / tpc;
        const int64_t wgs = n_qtiles * nslabs * nchunks, rounds = (wgs + Q_CUS - 1) / Q_CUS;
        const int64_t cost = rounds * tpc * (3 * nk + 4 * (nch < nk ? nch : nk));
        if (best_cost < 0 || cost < best_cost) {
            best_cost = cost;
            best = {(int)n_stiles, (int)n_qtiles, nch, (int)nslabs, (int)nchunks, (int)tpc};
        }
    }
    return best;
}

// The weights' gradient alone (gq == NULL): one slab and no second product, so a workgroup costs 3 d/32 per support tile
// -- the scores -- whatever the split, and a chunk's partials are B floats (glsp): nothing for the workspace to cap.
// Chunks only fill the chip: ceil(256 / n_qtiles) of them, at most the tile count; cost = rounds * tpc * 3 d/32.
BwdQueryPlan bwd_logw_plan(int64_t B, int64_t N, int row_chunks) {
    const int64_t n_stiles = (N + QBS - 1) / QBS, n_qtiles = (B + BQ - 1) / BQ;
    int64_t want = row_chunks > 0 ? row_chunks : (Q_CUS + n_qtiles - 1) / n_qtiles;
    if (want > n_stiles) want = n_stiles;
    const int64_t tpc = (n_stiles + want - 1) / want, nchunks = (n_stiles + tpc - 1) / tpc;
    return {(int)n_stiles, (int)n_qtiles, 1, 1, (int)nchunks, (int)tpc};
}

// dptab | tb | ascale | rqp | glsp | part | gap: the areas of the query gradient (`gq`: ascale, rqp, part), the chunks'
// logit-scale terms, and the query tiles' column sums of the weights' gradient (`gap`, when `gap_out` is asked for)
size_t bwd_query_layout(int64_t B, int64_t d, int64_t C, const BwdQueryPlan& p, char* base, BwdQueryWs* ws, bool gq = true,
                        float** gap_out = nullptr) {
    size_t off = 0;
    auto take = [&](size_t nfloat) {
        float* ptr = base ? reinterpret_cast<float*>(base + off) : nullptr;
        off += align256(nfloat * sizeof(float));
        return ptr;
    };
    BwdQueryWs w;
    w.dptab = take((size_t)B * C);
    w.tb = take((size_t)B);
    w.ascale = take(gq ? (size_t)p.nchunks * B : 0);
    w.rqp = take(gq ? (size_t)p.nchunks * B : 0);
    w.glsp = take((size_t)p.nchunks * B);
    w.part = take(gq ? (size_t)p.nchunks * B * d : 0);
    float* gap = take(gap_out ? (size_t)p.n_qtiles * QBS * p.n_stiles : 0);
    if (ws) *ws = w;
    if (gap_out) *gap_out = gap;
    return off;
}

template <int KIND, int NCH, bool WGT, int GA = 0>
int launch_bwd_query_kernel(const BwdQueryArgs& a, unsigned grid, hipStream_t st) {
    constexpr size_t LDS = GA ? Q_LDS_GA : (WGT ? Q_LDS_W : Q_LDS);
    static const bool attr = hipFuncSetAttribute(reinterpret_cast<const void*>(nw_bwd_query_kernel<KIND, NCH, WGT, GA>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS) == hipSuccess;
    if (!attr) return NW_ERR_LAUNCH;
    hipLaunchKernelGGL((nw_bwd_query_kernel<KIND, NCH, WGT, GA>), dim3(grid), dim3(TILE_THREADS), LDS, st, a);
    return NW_OK;
}
// ga: 0 -- gq alone; 1 -- gq and the weights' gradient; 2 -- the weights' gradient alone (the kernel's GA)
template <int KIND>
int launch_bwd_query_kind(const BwdQueryArgs& a, int nch, unsigned grid, hipStream_t st, int ga) {
    if (ga == 2) return launch_bwd_query_kernel<KIND, 1, true, 2>(a, grid, st);
    if (ga == 1) return nch == 8 ? launch_bwd_query_kernel<KIND, 8, true, 1>(a, grid, st) : launch_bwd_query_kernel<KIND, 4, true, 1>(a, grid, st);
    if (a.row_logw) return nch == 8 ? launch_bwd_query_kernel<KIND, 8, true>(a, grid, st) : launch_bwd_query_kernel<KIND, 4, true>(a, grid, st);
    return nch == 8 ? launch_bwd_query_kernel<KIND, 8, false>(a, grid, st) : launch_bwd_query_kernel<KIND, 4, false>(a, grid, st);
}

}  // namespace

bool bwd_query_shape_ok(int64_t B, int64_t N, int64_t d, int64_t C) {
    return bank_head_shape_ok(N, d, C) && B <= 0x7fffffffLL - BQ && N <= 0x7fffffffLL - QBS && C < (1 << 30);
}

size_t bwd_query_workspace_bytes(int64_t B, int64_t N, int64_t d, int64_t C, int row_chunks) {
    if (B <= 0 || !bwd_query_shape_ok(B, N, d, C)) return 0;
    return bwd_query_layout(B, d, C, bwd_query_plan(B, N, d, row_chunks), nullptr, nullptr);
}

size_t bwd_logw_workspace_bytes(int64_t B, int64_t N, int64_t d, int64_t C, int row_chunks, bool want_gq) {
    if (B <= 0 || !bwd_query_shape_ok(B, N, d, C)) return 0;
    float* gap;
    return bwd_query_layout(B, d, C, want_gq ? bwd_query_plan(B, N, d, row_chunks) : bwd_logw_plan(B, N, row_chunks), nullptr, nullptr,
                            want_gq, &gap);
}

// c.glogw: the weights' gradient as well (nw_bwd_query_logw_f32), with the plan, the areas and the launches of the query
// gradient when c.gq is set -- its bits are then those of the call without glogw -- and the weights-only plan when not
int launch_bwd_query(const BwdQueryCall& c) {
    hipStream_t st = c.st;
    const bool want_gq = c.gq != nullptr;
    const int ga = !c.glogw ? 0 : (want_gq ? 1 : 2);
    const BwdQueryPlan p = want_gq ? bwd_query_plan(c.B, c.N, c.d, c.row_chunks) : bwd_logw_plan(c.B, c.N, c.row_chunks);
    BwdQueryWs ws;
    float* gap = nullptr;
    const size_t need = bwd_query_layout(c.B, c.d, c.C, p, static_cast<char*>(c.workspace), &ws, want_gq, ga ? &gap : nullptr);
    if (!c.workspace || c.workspace_bytes < need) return NW_ERR_WORKSPACE;
    const int64_t wgs = (int64_t)p.n_qtiles * p.nslabs * p.nchunks;
    if (wgs > 0x7fffffffLL || (c.B * c.d / 4 + 255) / 256 > 0x7fffffffLL) return NW_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(nw_bwd_query_prologue_kernel, dim3((unsigned)c.B), dim3(256), 0, st, c.out, c.gout, ws.dptab, ws.tb, c.C);
    const BwdQueryArgs a = {c.q, c.s_split, c.s_scale, c.s_norm2, c.sy, c.row_lo, c.row_hi, c.lse, c.logit_scale_dev, c.row_logw, ws,
                            c.exclude, (int)c.B, (int)c.N, (int)c.d, (int)c.C, p.n_stiles, p.n_qtiles, p.nslabs, p.nchunks, p.tpc,
                            gap};
    int rc;
    switch (c.kind) {
        case NW_SCORE_EUCLIDEAN: rc = launch_bwd_query_kind<NW_SCORE_EUCLIDEAN>(a, p.nch, (unsigned)wgs, st, ga); break;
        case NW_SCORE_HYPERSPHERE: rc = launch_bwd_query_kind<NW_SCORE_HYPERSPHERE>(a, p.nch, (unsigned)wgs, st, ga); break;
        case NW_SCORE_COSINE: rc = launch_bwd_query_kind<NW_SCORE_COSINE>(a, p.nch, (unsigned)wgs, st, ga); break;
        case NW_SCORE_DOT: rc = launch_bwd_query_kind<NW_SCORE_DOT>(a, p.nch, (unsigned)wgs, st, ga); break;
        default: rc = launch_bwd_query_kind<NW_SCORE_CLIP>(a, p.nch, (unsigned)wgs, st, ga); break;
    }
    if (rc != NW_OK) return rc;
    if (want_gq)
        hipLaunchKernelGGL(nw_bwd_query_finish_kernel, dim3((unsigned)((c.B * c.d / 4 + 255) / 256)), dim3(256), 0, st, ws.part,
                           ws.rqp, ws.ascale, c.q, c.gq, p.nchunks, c.B, c.d);
    if (ga)
        hipLaunchKernelGGL(nw_bwd_logw_finish_kernel, dim3((unsigned)((c.N + 255) / 256)), dim3(256), 0, st, gap, c.glogw, p.n_qtiles,
                           (int64_t)p.n_stiles * QBS, c.N);
    if (c.glogit_scale) {
        if (c.kind == NW_SCORE_CLIP)
            hipLaunchKernelGGL(nw_bwd_query_gls_kernel, dim3(1), dim3(256), 0, st, ws.glsp, c.glogit_scale, p.nchunks, c.B);
        else if (hipMemsetAsync(c.glogit_scale, 0, 4, st) != hipSuccess)
            return NW_ERR_LAUNCH;
    }
    NW_CHECK_LAUNCH();
    return NW_OK;
}

}  // namespace nw
