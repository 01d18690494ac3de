// bwd_values_bank.hip -- gradient of the VALUE head w.r.t. the BANK ROWS over a resident split bank, without a (B,N) matrix
// (gfx950 / MI355X only; nw_bwd_values_bank_support_f32).
//
// The forward (fwd_values.hip) is out_b = sum_j W_bj v_j.  With g the (B,T) upstream gradient, the values and the weights
// constants and the bank rows the variable:
//     W_bj  = exp(score_bj + a_j - lse_b) on the rows the window admits, 0 elsewhere
//     c_bj  = g_b . v_j          (a T-long dot product, recomputed tile by tile on the matrix cores)
//     m_b   = g_b . out_b        (the prologue)
//     dS_bj = W_bj (c_bj - m_b)
//     (A_bj, r_bj) = bwd_pair_coeff<KIND>(raw score_bj, dS_bj, |s_j|^2, ...)            (the raw score, not score + a)
//     gs_j  = sum_b A_bj q_b + 2 (sum_b r_bj) s_j                                       (N, d)
// bwd_support.hip (the class head's gradient to the same rows) with its table lookup dP_b[y_j] - t_b replaced by c_bj - m_b;
// bwd_values.hip (this head's query gradient) with the contraction taken over the queries instead of the rows.  A workgroup
// owns one 64-row support tile, a slab of 32 * NCH columns of d and a contiguous chunk of the 64-query tiles.  Per query
// tile it
//   1. recomputes the tile's dot products (tile_dots_f16x2<4, true>: raw queries split in registers, split bank rows);
//   2. behind a barrier (the ring of the first product must be dead) computes c with the same routine over (gout, the split
//      value rows, T) on the same ring, as bwd_values.hip step 2 does: the raw gout rows are split in registers, their row
//      statistics go to header arrays of their own (gn2, gsc), the value rows' scales are in vsc, the ring's rotation is
//      qt % (T / 32).  Both accumulators have the layout "query on the lane, rows 16r + 4g + e in the registers", so
//      c = acc2 gsc_b vsc_j meets W element for element with no exchange;
//   3. the consumer waves turn both into A in registers -- the forward's window rule, the weighted W, dS, the kind's
//      derivative --, add r to 16 per-lane fp32 sums and give the wave's largest |A| to LDS;
//   4. from there on bwd_support.hip's steps 3 and 4: the workgroup's running exponent with its exact rescale, A 2^E as fp16
//      halves h + l in LDS, gs_tile += A^T Q on v_mfma_f32_16x16x32_f16 over the packed q on all EIGHT waves (lh + hl + hh).
// Scaling, the error of the contraction and the chunks are bwd_support.hip's (its header spells them out): with Amax the
// tile's largest |A|,
//     |error of gs_jk| <~ (2^-21 + B 2^-24) sum_b |A_bj| |q_bk| + 2^-38 (Amax sum_b |q_bk| + max|q| sum_b |A_bj|) + fp32 rounding of 2 r s
// on top of the error A itself carries: c - m cancels, and the error of c is ~2.4e-7 sum_t |g_t v_jt| (tile_f16.h) whatever
// the spread of the values among the rows, so value columns with a large common offset lose that many bits of the gradient.
// Centre such columns.
// Scaling gout by 2^k scales gs exactly: gsc_b and m_b follow it, acc2 does not move, and A's exponent moves by k.
// Exact zeros: a row at a = -inf, a row no query's window admits, a dead query (lse = -inf), a row past N and a lane past B
// have W = 0, so dS = A = r = +-0 -- the value rows must be FINITE in every row, the forward's condition: c of a pair that
// takes no part is multiplied with W = 0 --; both halves are zeros and +0 + (+-0) = +0 in every accumulator.  A tile of
// zeros leaves the exponent alone; the coefficients of an all-zero query, which multiply zeros, are zeros too.
// Each chunk writes its tile still scaled, with the exponent beside it -- into gs itself when there is one chunk --; the
// finish kernel unscales, adds the chunks in ascending order from +0 and adds 2 r s.  No float atomics: two calls give the
// same bits.
// The skeleton, the running exponent, the store, the finish kernel and the workspace areas behind m are bwd_support_core.h's.
#include "bwd_support_core.h"
#include "bwd_coeff.h"
#include "fused_plan.h"   // NW_FOR_EACH_KIND

namespace nw {
namespace {

// qn2[BQ] | qsc[BQ] | gn2[BQ] | gsc[BQ] | sn2[SBS] | ssc[SBS] | vsc[SBS] | law[SBS] | wmx[NCONS]
constexpr int S_HDR = (4 * BQ + 4 * SBS + NCONS) * 4;
static_assert(S_HDR % 16 == 0, "stage buffers must stay 16-byte aligned");
constexpr size_t S_LDS = S_HDR + DmaCfg<SRS>::STAGE_BYTES;
static_assert(S_LDS <= 80 * 1024, "header + ring exceed the LDS of two workgroups per CU");

struct SupWs : SupRowsWs {   // the prologue's m in front of the areas every gradient to the rows has
    float* mb;
};
struct SupArgs {
    const float *q, *s, *s_scale, *s_norm2, *v, *v_scale, *gout;
    const int *win_lo, *win_hi;
    const float *lse, *logit_scale, *row_logw;
    float* gs_out;     // gs, or the partial tiles
    SupWs ws;
    int exclude, B, N, d, T, n_stiles, n_qtiles, nslabs, nchunks, tpc;
};

// m_b = g_b . out_b (as nw_bwd_values_prologue_kernel: a thread adds its columns in order, the block in a fixed tree) and
// max_k |q_bk|: one workgroup per query.
__global__ __launch_bounds__(256) void nw_bwd_values_bank_prologue_kernel(const float* __restrict__ out,
                                                                           const float* __restrict__ gout,
                                                                           const float* __restrict__ q, float* __restrict__ mb,
                                                                           float* __restrict__ qmax, int64_t T, int64_t d) {
    __shared__ float red[8];
    const int64_t b = blockIdx.x;
    float t = 0.f, mx = 0.f;
    for (int64_t c = threadIdx.x; c < T; c += 256) t = __builtin_fmaf(gout[b * T + c], out[b * T + c], t);
    for (int64_t k = threadIdx.x; k < d; k += 256) mx = fmaxf(mx, fabsf(q[b * d + k]));
    t = block_sum(t, red);
    mx = block_max(mx, red);
    if (threadIdx.x == 0) mb[b] = t, qmax[b] = mx;
}

template <int KIND, int NCH>
__global__ __launch_bounds__(TILE_THREADS, 2) void nw_bwd_values_bank_support_kernel(const SupArgs a) {
    constexpr bool NEED_NORM = (KIND != NW_SCORE_DOT);
    constexpr float LN2 = 0.693147180559945309417f;
    constexpr int NCC = NCH / 2;     // 32-column chunks per wave
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* qn2 = reinterpret_cast<float*>(smem);
    float* qsc_s = qn2 + BQ;
    float* gn2 = qsc_s + BQ;         // the second product's row statistics: |g_b|^2 (not used) ...
    float* gsc_s = gn2 + BQ;         // ... and the gout rows' 2^-e_b
    float* sn2 = gsc_s + BQ;
    float* ssc = sn2 + SBS;
    float* vsc = ssc + SBS;          // the value rows' 2^-e_j
    float* law = vsc + SBS;          // the tile's row log-weights (0 without them: the fused multiply-add is then exact)
    float* wmx = law + SBS;          // the consumer waves' largest |A| of the query tile
    float4* stage = reinterpret_cast<float4*>(smem + S_HDR);
    _Float16* Ahs = reinterpret_cast<_Float16*>(smem + S_HDR);
    _Float16* Als = Ahs + SBS * X_STRIDE;
    float* pmx = reinterpret_cast<float*>(smem + S_HDR);   // the r exchange at the end, over the same bytes

    const int B = a.B, N = a.N, d = a.d, T = a.T;
    const int tid = threadIdx.x, lane = tid & 63, i = lane & 15, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // workgroup -> (chunk, support tile, slab): the workgroups that share a tile's bank rows are neighbours
    const int slab = blockIdx.x % a.nslabs, rest = blockIdx.x / a.nslabs;
    const int stile = rest % a.n_stiles, chunk = rest / a.n_stiles;
    const int s0 = stile * SBS;
    const int nk = d / BK, nkt = T / BK, ncb = d / 16;
    const int kc0 = slab * NCH;
    const int nc = min(NCH, nk - kc0);                 // 32-column chunks of this slab
    const int qt_begin = chunk * a.tpc, qt_end = min(a.n_qtiles, qt_begin + a.tpc);
    const int rb = wave & 3, hf = wave >> 2;          // the third product: rows 16 rb .. + 15, chunks hf, hf + 2, ...
    const bool weighted = a.row_logw != nullptr;
    const bool exclude = a.exclude != 0;

    // the support tile is the workgroup's own: its header is staged once
    for (int t = tid; t < SBS; t += TILE_THREADS) {
        const int j = min(s0 + t, N - 1);
        if (NEED_NORM) sn2[t] = a.s_norm2[j];
        ssc[t] = a.s_scale[j];
        vsc[t] = a.v_scale[j];
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
    const int tile_end = s0 + SBS < N ? s0 + SBS : N;
    int Erun = 0;          // the workgroup's exponent in this chunk so far (uniform); `have`: some query tile has set it
    bool have = false;

    for (int qt = qt_begin; qt < qt_end; ++qt) {
        const int q0 = qt * BQ;
        f32x4 acc[SRS], acc2[SRS];
        tile_dots_f16x2<SRS, true>(a.q, a.s, B, N, d, q0, s0, stage, acc, qt % nk, qn2, qsc_s);
        __syncthreads();   // the ring of the first product is dead
        tile_dots_f16x2<SRS, true>(a.gout, a.v, B, N, T, q0, s0, stage, acc2, qt % nkt, gn2, gsc_s);
        __syncthreads();   // the header is visible, the ring is dead

        float xr[SRS][4];
        if (wave < NCONS) {
            // ================================ consumers: A in registers, its r sums, its maximum ================================
            const int qrow = 16 * wave + i;
            const float qn = NEED_NORM ? qn2[qrow] : 0.f;
            const float gsc = gsc_s[qrow];
            float scale, nq, inq2;
            bwd_query_factors<KIND>(qn, a.logit_scale, scale, nq, inq2);
            const SupQuery Q = sup_query<KIND>(a.lse, a.win_lo, a.win_hi, exclude, B, N, q0, qrow, g, s0, tile_end, qn,
                                               qsc_s[qrow], scale);
            const float mq = a.ws.mb[Q.bb];
            // an all-zero query adds nothing to A^T Q whatever its coefficients are, and those of the cosine kinds are of the
            // order 1 / NW_NORM_EPS there: they are kept away from the exponent (bwd_support.hip)
            const bool qzero = a.ws.qmax[Q.bb] == 0.f;
            float amax = 0.f, rq_unused = 0.f, gls_unused = 0.f;
#pragma unroll
            for (int r = 0; r < SRS; ++r) {
                float4 n4 = make_float4(0.f, 0.f, 0.f, 0.f);
                if (NEED_NORM) n4 = *reinterpret_cast<const float4*>(sn2 + 16 * r + 4 * g);
                const float4 s4 = *reinterpret_cast<const float4*>(ssc + 16 * r + 4 * g);
                const float4 v4 = *reinterpret_cast<const float4*>(vsc + 16 * r + 4 * g);
                const float4 a4 = *reinterpret_cast<const float4*>(law + 16 * r + 4 * g);
                const float nn[4] = {n4.x, n4.y, n4.z, n4.w}, ss[4] = {s4.x, s4.y, s4.z, s4.w};
                const float vs[4] = {v4.x, v4.y, v4.z, v4.w}, aw[4] = {a4.x, a4.y, a4.z, a4.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    // the weighted score goes into W alone: bwd_pair_coeff takes the raw score u (bwd_query.hip)
                    float u;
                    const float W = sup_weight<KIND>(Q, acc[r][e], nn[e], ss[e], aw[e], 16 * r + e, B, N, u);
                    const float cv = acc2[r][e] * (gsc * vs[e]);   // both scales are powers of two: exact
                    const float dS = W * (cv - mq);
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

        const float factor = sup_running_exponent(wmx, Erun, have);
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

    // ---- results, still scaled
    sup_rows_store<NCC>(gacc, a.gs_out + (size_t)chunk * N * d, N, d, s0, kc0, nc, rb, hf, lane);
    if (slab == 0) {   // (uniform over the workgroup: every slab holds the same r sums and the same exponent)
        if (tid == 0) a.ws.esc[(size_t)chunk * a.n_stiles + stile] = -(Erun + *a.ws.qexp);
        sup_row_sums(pm, pmx, a.ws.rp + (size_t)chunk * ((size_t)a.n_stiles * SBS) + s0, tid, wave);
    }
}

// mb | qmax | qexp | qpack | rp | esc | part: nothing of size B x N, nothing of size N x T
size_t sup_layout(int64_t B, int64_t N, int64_t d, const SupPlan& p, char* base, SupWs* ws) {
    SupCarve ws_{base};
    SupWs w;
    w.mb = ws_.take<float>((size_t)B * 4);
    sup_rows_layout(ws_, B, N, d, p, w);
    if (ws) *ws = w;
    return ws_.off;
}

}  // namespace

size_t bwd_values_bank_support_workspace_bytes(int64_t B, int64_t N, int64_t d, int64_t T, int query_chunks) {
    if (B <= 0 || !fwd_values_shape_ok(B, N, d, T)) return 0;
    return sup_layout(B, N, d, sup_plan(B, N, d, query_chunks), nullptr, nullptr);
}

int launch_bwd_values_bank_support(const BwdValuesBankSupportCall& c) {
    hipStream_t st = c.st;
    const SupPlan p = sup_plan(c.B, c.N, c.d, c.query_chunks);
    SupWs ws;
    const size_t need = sup_layout(c.B, c.N, c.d, p, static_cast<char*>(c.workspace), &ws);
    if (!c.workspace || c.workspace_bytes < need) return NW_ERR_WORKSPACE;
    const int64_t wgs = (int64_t)p.n_stiles * p.nslabs * p.nchunks;
    if (!sup_rows_grids_ok(p, c.N, c.d)) return NW_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(nw_bwd_values_bank_prologue_kernel, dim3((unsigned)c.B), dim3(256), 0, st, c.out, c.gout, c.q, ws.mb, ws.qmax,
                       c.T, c.d);
    launch_sup_pack(c.q, ws.qmax, ws.qexp, ws.qpack, c.B, c.d, p, st);
    float* part = p.nchunks > 1 ? ws.part : c.gs;
    const SupArgs a = {c.q, c.s_split, c.s_scale, c.s_norm2, c.v_split, c.v_scale, c.gout, c.row_lo, c.row_hi, c.lse,
                       c.logit_scale_dev, c.row_logw, part, ws, c.row_lo && c.exclude != 0, (int)c.B, (int)c.N, (int)c.d, (int)c.T,
                       p.n_stiles, p.n_qtiles, p.nslabs, p.nchunks, p.tpc};
    int rc = NW_ERR_UNSUPPORTED;   // (the entry admits the five kinds alone)
#define NW_KIND_CASE(K)                                                                                                         \
    case K:                                                                                                                     \
        rc = launch_sup_kind<nw_bwd_values_bank_support_kernel<K, S_NCH_MAX>, nw_bwd_values_bank_support_kernel<K, S_NCH_MIN>>( \
            a, S_LDS, p.nch, (unsigned)wgs, st);                                                                                \
        break;
    switch (c.kind) { NW_FOR_EACH_KIND(NW_KIND_CASE) }
#undef NW_KIND_CASE
    if (rc != NW_OK) return rc;
    launch_sup_rows_finish(part, ws, c.s, c.gs, p, c.N, c.d, st);
    NW_CHECK_LAUNCH();
    return NW_OK;
}

}  // namespace nw
