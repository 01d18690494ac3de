// bwd_support.hip -- gradient of the CLASS head w.r.t. the BANK ROWS over a resident split bank, without a (B,N) matrix
// (gfx950 / MI355X only; nw_bwd_bank_support_f32).
//
// backward.hip's closed form with the bank rows the variable (bwd_query.hip has the queries in that place):
//     W_bj  = exp(score_bj + a_j - lse_b) on the rows the window admits, 0 elsewhere
//     dP_bc = g_bc exp(-out_bc) (an absent class left out), t_b = sum_c dP_bc P_bc      (the prologue, no pass over the bank)
//     dS_bj = W_bj (dP_b[y_j] - t_b)
//     (A_bj, r_bj) = bwd_pair_coeff<KIND>(raw score_bj, dS_bj, |s_j|^2, ...)            (the raw score, not score + a)
//     gs_j  = sum_b A_bj q_b + 2 (sum_b r_bj) s_j                                       (N, d)
// A contraction over the QUERIES of a coefficient matrix that is recomputed tile by tile: bwd_values_support.hip's skeleton
// with bwd_query.hip's coefficient where that kernel has W.  A workgroup owns one 64-row support tile, a slab of 32 * NCH
// columns of d and a contiguous chunk of the 64-query tiles.  Per query tile it
//   1. recomputes the tile's dot products (tile_dots_f16x2<4, true>: raw queries split in registers, split bank rows);
//   2. the consumer waves turn them into A in registers -- the forward's window rule, the weighted W, dW gathered from the
//      (B,C) table of the prologue, dS, the kind's derivative -- add r to 16 per-lane fp32 sums and give the wave's largest
//      |A| to LDS;
//   3. behind a barrier every thread takes the tile's largest |A| and with it the workgroup's running exponent (below); the
//      consumers split A 2^E into fp16 halves h + l and write them to LDS as [row][query] (144-byte rows);
//   4. all EIGHT waves run gs_tile += A^T Q on v_mfma_f32_16x16x32_f16, K = the query, in the order lh + hl + hh.  The B
//      operand comes from global memory: a prologue packs q once per call, split and in MFMA lane order (B x d x 4 bytes).
// Scaling.  A is signed and has no a-priori bound for the distance kinds (1/D).  The exponent belongs to the WORKGROUP: E is
// the split exponent of the largest |A| the support tile has shown so far in the chunk, over all its 64 rows; when a query
// tile raises the maximum, every accumulator of the workgroup is multiplied by the power of two between the old and the new
// exponent (exact) before the tile is added.  An element of A keeps 22 bits down to 2^-28 of the tile's running maximum and
// an absolute error of 2^-40 of it below.  q is split against ONE exponent, that of max |q| (a maximum: the same whatever
// the order).  Products are exact, sums are fp32; with Amax the tile's largest |A|:
//     |error of gs_jk| <~ (2^-21 + B 2^-24) sum_b |A_bj| |q_bk| + 2^-38 (Amax sum_b |q_bk| + max|q| sum_b |A_bj|) + fp32 rounding of 2 r s
// Scaling gout by 2^k moves E by k and nothing else: gs scales exactly.
// Exact zeros: a row at a = -inf, a row no query's window admits, a dead query (lse = -inf), a row past N and a lane past B
// have W = 0, so dS = A = r = +-0: both halves are zeros and +0 + (+-0) = +0 in every accumulator.  A tile of zeros leaves
// the exponent alone (split_exponent is never asked about 0); the coefficients of an all-zero query, which multiply zeros,
// are zeros too.
// Query chunks fill the chip when there are few support tiles.  Each writes its tile still scaled, with the exponent beside
// it -- into gs itself when there is one chunk --; the finish kernel unscales, adds the chunks in ascending order from +0
// and adds 2 r s.  No float atomics: two calls give the same bits.
// The skeleton -- plan, q's exponent and pack, the window rule and W, the h + l write, the MFMA block, the exchange of the r
// sums, the launch -- is bwd_support_core.h's, shared with bwd_values_support.hip; X there is A here.
#include "bwd_support_core.h"
#include "bwd_coeff.h"
#include "fused_plan.h"   // NW_FOR_EACH_KIND

namespace nw {
namespace {

// qn2[BQ] | qsc[BQ] | sn2[SBS] | ssc[SBS] | law[SBS] | lab[SBS] | wmx[NCONS]
constexpr int S_HDR = (2 * BQ + 4 * SBS + NCONS) * 4;
static_assert(S_HDR % 16 == 0, "stage buffers must stay 16-byte aligned");
constexpr size_t S_LDS = S_HDR + DmaCfg<SRS>::STAGE_BYTES;
static_assert(S_LDS <= 80 * 1024, "header + ring exceed the LDS of two workgroups per CU");

struct SupWs {
    float *dptab, *tb, *qmax;
    int* qexp;
    half8* qpack;      // [query tile][16-column block][32-query step][h, l][lane]: 8 halves each
    float* rp;         // [chunk][row]: rows padded to the tile
    int* esc;          // [chunk][support tile]: the exponent that unscales the chunk's tile
    float* part;       // [chunk][N][d], only with more than one chunk
};
struct SupArgs {
    const float *q, *s, *s_scale, *s_norm2;
    const int64_t* sy;
    const int *win_lo, *win_hi;
    const float *lse, *logit_scale, *row_logw;
    float* gs_out;     // gs, or the partial tiles
    SupWs ws;
    int exclude, B, N, d, C, n_stiles, n_qtiles, nslabs, nchunks, tpc;
};

// dP (B,C), t_b and max_k |q_bk|: one workgroup per query.  (bwd_query.hip's prologue, which that file keeps to itself,
// with the maximum beside it.  The block sum runs in a fixed order: deterministic.)
__global__ __launch_bounds__(256) void nw_bwd_bank_support_prologue_kernel(const float* __restrict__ out,
                                                                            const float* __restrict__ gout,
                                                                            const float* __restrict__ q, float* __restrict__ dptab,
                                                                            float* __restrict__ tb, float* __restrict__ qmax,
                                                                            int64_t C, int64_t d) {
    __shared__ float red[8];
    const int64_t b = blockIdx.x;
    // what the forward's logf gives for an empty class, from the same routine (blockIdx.y is 0: not folded on the host)
    const float absent = logf((float)blockIdx.y + NW_LOG_EPS);
    float t = 0.f, mx = 0.f;
    for (int64_t c = threadIdx.x; c < C; c += 256) {
        const float o = out[b * C + c];
        float dp = 0.f;
        if (o > absent) {
            dp = gout[b * C + c] * expf(-o);
            t += dp * (expf(o) - NW_LOG_EPS);
        }
        dptab[b * C + c] = dp;
    }
    for (int64_t k = threadIdx.x; k < d; k += 256) mx = fmaxf(mx, fabsf(q[b * d + k]));
    t = block_sum(t, red);
    mx = block_max(mx, red);
    if (threadIdx.x == 0) tb[b] = t, qmax[b] = mx;
}

template <int KIND, int NCH>
__global__ __launch_bounds__(TILE_THREADS, 2) void nw_bwd_bank_support_kernel(const SupArgs a) {
    constexpr bool NEED_NORM = (KIND != NW_SCORE_DOT);
    constexpr float LN2 = 0.693147180559945309417f;
    constexpr int NCC = NCH / 2;     // 32-column chunks per wave
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* qn2 = reinterpret_cast<float*>(smem);
    float* qsc_s = qn2 + BQ;
    float* sn2 = qsc_s + BQ;
    float* ssc = sn2 + SBS;
    float* law = ssc + SBS;          // the tile's row log-weights (0 without them: the fused multiply-add is then exact)
    int* lab = reinterpret_cast<int*>(law + SBS);   // the tile's labels, -1 outside [0, C)
    float* wmx = reinterpret_cast<float*>(lab + SBS);   // the consumer waves' largest |A| of the query tile
    float4* stage = reinterpret_cast<float4*>(smem + S_HDR);
    _Float16* Ahs = reinterpret_cast<_Float16*>(smem + S_HDR);
    _Float16* Als = Ahs + SBS * X_STRIDE;
    float* pmx = reinterpret_cast<float*>(smem + S_HDR);   // the r exchange at the end, over the same bytes

    const int B = a.B, N = a.N, d = a.d;
    const int tid = threadIdx.x, lane = tid & 63, i = lane & 15, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // workgroup -> (chunk, support tile, slab): the workgroups that share a tile's bank rows are neighbours
    const int slab = blockIdx.x % a.nslabs, rest = blockIdx.x / a.nslabs;
    const int stile = rest % a.n_stiles, chunk = rest / a.n_stiles;
    const int s0 = stile * SBS;
    const int nk = d / BK, ncb = d / 16;
    const int kc0 = slab * NCH;
    const int nc = min(NCH, nk - kc0);                 // 32-column chunks of this slab
    const int qt_begin = chunk * a.tpc, qt_end = min(a.n_qtiles, qt_begin + a.tpc);
    const int rb = wave & 3, hf = wave >> 2;          // the second product: rows 16 rb .. + 15, chunks hf, hf + 2, ...
    const bool weighted = a.row_logw != nullptr;
    const bool exclude = a.exclude != 0;

    // the support tile is the workgroup's own: its header is staged once
    for (int t = tid; t < SBS; t += TILE_THREADS) {
        const int j = min(s0 + t, N - 1);
        if (NEED_NORM) sn2[t] = a.s_norm2[j];
        ssc[t] = a.s_scale[j];
        law[t] = weighted ? a.row_logw[j] : 0.f;
        const int64_t y = a.sy[j];
        lab[t] = ((uint64_t)y < (uint64_t)a.C) ? (int)y : -1;
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
    const int tile_end = s0 + SBS < N ? s0 + SBS : N;
    int Erun = 0;          // the workgroup's exponent in this chunk so far (uniform); `have`: some query tile has set it
    bool have = false;

    for (int qt = qt_begin; qt < qt_end; ++qt) {
        const int q0 = qt * BQ;
        f32x4 acc[SRS];
        tile_dots_f16x2<SRS, true>(a.q, a.s, B, N, d, q0, s0, stage, acc, qt % nk, qn2, qsc_s);
        __syncthreads();   // the ring is dead

        float xr[SRS][4];
        if (wave < NCONS) {
            // ================================ consumers: A in registers, its r sums, its maximum ================================
            const int qrow = 16 * wave + i;
            const float qn = NEED_NORM ? qn2[qrow] : 0.f;
            float scale, nq, inq2;
            bwd_query_factors<KIND>(qn, a.logit_scale, scale, nq, inq2);
            const SupQuery Q = sup_query<KIND>(a.lse, a.win_lo, a.win_hi, exclude, B, N, q0, qrow, g, s0, tile_end, qn,
                                               qsc_s[qrow], scale);
            const float tq = a.ws.tb[Q.bb];
            // an all-zero query adds nothing to A^T Q whatever its coefficients are, and those of the cosine kinds are of the
            // order 1 / NW_NORM_EPS there: they are kept away from the exponent
            const bool qzero = a.ws.qmax[Q.bb] == 0.f;
            const float* dprow = a.ws.dptab + (size_t)Q.bb * a.C;
            float dw[SRS][4], amax = 0.f, rq_unused = 0.f, gls_unused = 0.f;
#pragma unroll
            for (int r = 0; r < SRS; ++r) {
                const int4 y4 = *reinterpret_cast<const int4*>(lab + 16 * r + 4 * g);
                const int yy[4] = {y4.x, y4.y, y4.z, y4.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) dw[r][e] = dprow[yy[e] < 0 ? 0 : yy[e]];
#pragma unroll
                for (int e = 0; e < 4; ++e) dw[r][e] = yy[e] < 0 ? 0.f : dw[r][e];
            }
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
                    // the weighted score goes into W alone: bwd_pair_coeff takes the raw score u (bwd_query.hip)
                    float u;
                    const float W = sup_weight<KIND>(Q, acc[r][e], nn[e], ss[e], aw[e], 16 * r + e, B, N, u);
                    const float dS = W * (dw[r][e] - tq);
                    float av, rs;
                    bwd_pair_coeff<KIND>(u * LN2, dS, nn[e], scale, nq, inq2, av, rs, rq_unused, gls_unused);
                    // (an all-zero query has the unit vector 0 and cos = 0; the distance, 1, says 1/2: no share of df/d|s|^2)
                    if (KIND == NW_SCORE_HYPERSPHERE && qzero) rs = 0.f;
                    pm[r][e] += rs;
                    xr[r][e] = qzero ? 0.f : av;
                    amax = fmaxf(amax, fabsf(xr[r][e]));
                }
            }
            // the wave's maximum (a maximum: the same whatever the order)
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o));
            if (lane == 0) wmx[wave] = amax;
        }
        __syncthreads();   // the four maxima are in LDS

        // ---- the workgroup's exponent: raised (a smaller E) when this query tile holds a larger coefficient than any before
        float factor = 1.f;
        {
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
        }
        if (wave < NCONS) {
            const int qrow = 16 * wave + i;
            const float up = __builtin_ldexpf(1.f, Erun);
#pragma unroll
            for (int r = 0; r < SRS; ++r)
#pragma unroll
                for (int e = 0; e < 4; ++e) sup_put_halves(Ahs, Als, 16 * r + 4 * g + e, qrow, xr[r][e], up, -HALF_MAX);
        }
        if (factor != 1.f) {   // (uniform over the workgroup)
#pragma unroll
            for (int c = 0; c < NCC; ++c) {
                gacc[c][0] *= factor;
                gacc[c][1] *= factor;
            }
        }
        __syncthreads();   // A is in LDS

        // ================================ all waves: gs tile += A^T Q ================================
        sup_mfma_tile<NCC>(gacc, Ahs, Als, a.ws.qpack, qt, ncb, kc0, nc, rb, hf, lane);
        __syncthreads();   // the ring is free for the next tile
    }

    // ---- results, still scaled: gacc[cc][nb][e] of lane (i, g) = gs'[row 16 rb + 4g + e][column 32 (kc0 + 2 cc + hf) + 16 nb + i]
#pragma unroll
    for (int cc = 0; cc < NCC; ++cc) {
        const int c = 2 * cc + hf;
        if (c < nc) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int row = s0 + 16 * rb + 4 * g + e;
                if (row < N) {
                    float* dst = a.gs_out + (size_t)chunk * N * d + (size_t)row * d + (size_t)(kc0 + c) * BK + i;
                    dst[0] = gacc[cc][0][e];
                    dst[16] = gacc[cc][1][e];
                }
            }
        }
    }
    if (slab == 0) {   // (uniform over the workgroup: every slab holds the same r sums and the same exponent)
        if (tid == 0) a.ws.esc[(size_t)chunk * a.n_stiles + stile] = -(Erun + *a.ws.qexp);
        sup_row_sums(pm, pmx, a.ws.rp + (size_t)chunk * ((size_t)a.n_stiles * SBS) + s0, tid, wave);
    }
}

// gs[j,k] = sum_chunks part[c][j,k] 2^esc[c][tile of j] + 2 (sum_chunks rp[c][j]) s[j,k], chunks in ascending order from +0
// (k in float4s).  With one chunk `part` is gs itself: a thread reads and writes its own four floats.
__global__ __launch_bounds__(256) void nw_bwd_bank_support_finish_kernel(const float* part, const int* __restrict__ esc,
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

// dptab | tb | qmax | qexp | qpack | rp | esc | part
size_t sup_layout(int64_t B, int64_t N, int64_t d, int64_t C, const SupPlan& p, char* base, SupWs* ws) {
    SupCarve ws_{base};
    const size_t npad = (size_t)p.n_stiles * SBS;
    SupWs w;
    w.dptab = ws_.take<float>((size_t)B * C * 4);
    w.tb = ws_.take<float>((size_t)B * 4);
    w.qmax = ws_.take<float>((size_t)B * 4);
    w.qexp = ws_.take<int>(4);
    w.qpack = ws_.take<half8>((size_t)p.n_qtiles * BQ * d * 4);
    w.rp = ws_.take<float>((size_t)p.nchunks * npad * 4);
    w.esc = ws_.take<int>((size_t)p.nchunks * p.n_stiles * 4);
    w.part = ws_.take<float>(p.nchunks > 1 ? (size_t)p.nchunks * N * d * 4 : 0);
    if (ws) *ws = w;
    return ws_.off;
}

}  // namespace

size_t bwd_bank_support_workspace_bytes(int64_t B, int64_t N, int64_t d, int64_t C, int query_chunks) {
    if (B <= 0 || !bwd_query_shape_ok(B, N, d, C)) return 0;
    return sup_layout(B, N, d, C, sup_plan(B, N, d, query_chunks), nullptr, nullptr);
}

int launch_bwd_bank_support(const BwdBankSupportCall& c) {
    hipStream_t st = c.st;
    const SupPlan p = sup_plan(c.B, c.N, c.d, c.query_chunks);
    SupWs ws;
    const size_t need = sup_layout(c.B, c.N, c.d, c.C, p, static_cast<char*>(c.workspace), &ws);
    if (!c.workspace || c.workspace_bytes < need) return NW_ERR_WORKSPACE;
    const int64_t wgs = (int64_t)p.n_stiles * p.nslabs * p.nchunks;
    const int64_t npack = sup_pack_threads(p, c.d), total4 = c.N * c.d / 4;
    if (wgs > 0x7fffffffLL || (npack + 255) / 256 > 0x7fffffffLL || (total4 + 255) / 256 > 0x7fffffffLL) return NW_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(nw_bwd_bank_support_prologue_kernel, dim3((unsigned)c.B), dim3(256), 0, st, c.out, c.gout, c.q, ws.dptab,
                       ws.tb, ws.qmax, c.C, c.d);
    launch_sup_pack(c.q, ws.qmax, ws.qexp, ws.qpack, c.B, c.d, p, st);
    float* part = p.nchunks > 1 ? ws.part : c.gs;
    const SupArgs a = {c.q, c.s_split, c.s_scale, c.s_norm2, c.sy, c.row_lo, c.row_hi, c.lse, c.logit_scale_dev, c.row_logw, part, ws,
                       c.row_lo && c.exclude != 0, (int)c.B, (int)c.N, (int)c.d, (int)c.C, p.n_stiles, p.n_qtiles, p.nslabs,
                       p.nchunks, p.tpc};
    int rc = NW_ERR_UNSUPPORTED;   // (the entry admits the five kinds alone)
#define NW_KIND_CASE(K)                                                                                           \
    case K:                                                                                                       \
        rc = launch_sup_kind<nw_bwd_bank_support_kernel<K, S_NCH_MAX>, nw_bwd_bank_support_kernel<K, S_NCH_MIN>>( \
            a, S_LDS, p.nch, (unsigned)wgs, st);                                                                  \
        break;
    switch (c.kind) { NW_FOR_EACH_KIND(NW_KIND_CASE) }
#undef NW_KIND_CASE
    if (rc != NW_OK) return rc;
    hipLaunchKernelGGL(nw_bwd_bank_support_finish_kernel, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, st, part, ws.esc,
                       ws.rp, c.s, c.gs, p.nchunks, p.n_stiles, c.N, c.d);
    NW_CHECK_LAUNCH();
    return NW_OK;
}

}  // namespace nw
