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
// The skeleton -- plan, gout's exponent and pack, the window rule and W, the h + l write, the MFMA block, the exchange of the
// W m sums, the launch -- is bwd_support_core.h's, shared with bwd_support.hip; X there is W here.
#include "bwd_support_core.h"
#include "fused_plan.h"   // NW_FOR_EACH_KIND

namespace nw {
namespace {

// qn2[BQ] | qsc[BQ] | sn2[SBS] | ssc[SBS] | law[SBS]
constexpr int S_HDR = (2 * BQ + 3 * SBS) * 4;
static_assert(S_HDR % 16 == 0, "stage buffers must stay 16-byte aligned");
constexpr size_t S_LDS = S_HDR + DmaCfg<SRS>::STAGE_BYTES;
static_assert(S_LDS <= 80 * 1024, "header + ring exceed the LDS of two workgroups per CU");
constexpr int W_SHIFT = 15;       // W 2^15 <= 32768: inside fp16

struct SupWs {
    float *mb, *gmax;
    int* gexp;
    half8* gpack;      // [query tile][16-column block][32-query step][h, l][lane]: 8 halves each
    float *glp, *pmp;  // [chunk][slab, wave half][row], [chunk][row]: rows padded to the tile
    float* part;       // [chunk][N][T], only with gvalues and more than one chunk
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

template <int KIND, int NCH>
__global__ __launch_bounds__(TILE_THREADS, 2) void nw_bwd_values_support_kernel(const SupArgs a) {
    constexpr bool NEED_NORM = (KIND != NW_SCORE_DOT);
    constexpr int NCC = NCH / 2;     // 32-column chunks per wave
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* qn2 = reinterpret_cast<float*>(smem);
    float* qsc_s = qn2 + BQ;
    float* sn2 = qsc_s + BQ;
    float* ssc = sn2 + SBS;
    float* law = ssc + SBS;          // the tile's row log-weights (0 without them: the fused multiply-add is then exact)
    float4* stage = reinterpret_cast<float4*>(smem + S_HDR);
    _Float16* Wh = reinterpret_cast<_Float16*>(smem + S_HDR);
    _Float16* Wl = Wh + SBS * X_STRIDE;
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
            const int qrow = 16 * wave + i;
            const SupQuery Q = sup_query<KIND>(a.lse, a.win_lo, a.win_hi, exclude, B, N, q0, qrow, g, s0, tile_end,
                                               NEED_NORM ? qn2[qrow] : 0.f, qsc_s[qrow], scale);
            const float mq = a.ws.mb[Q.bb];
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
                    float u;
                    const float W = sup_weight<KIND>(Q, acc[r][e], nn[e], ss[e], aw[e], 16 * r + e, B, N, u);
                    pm[r][e] = __builtin_fmaf(W, mq, pm[r][e]);
                    sup_put_halves(Wh, Wl, 16 * r + 4 * g + e, qrow, W, (float)(1 << W_SHIFT), 0.f);
                }
            }
        }
        __syncthreads();   // W is in LDS

        // ================================ all waves: gV tile += W^T G ================================
        sup_mfma_tile<NCC>(gacc, Wh, Wl, a.ws.gpack, qt, ncb, kc0, nc, rb, hf, lane);
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
        if (want_pm) sup_row_sums(pm, pmx, a.ws.pmp + (size_t)chunk * npad + s0, tid, wave);   // (uniform over the workgroup)
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

// mb | gmax | gexp | gpack | glp | pmp | part
size_t sup_layout(int64_t B, int64_t N, int64_t T, const SupPlan& p, bool want_gvalues, char* base, SupWs* ws) {
    SupCarve ws_{base};
    const size_t npad = (size_t)p.n_stiles * SBS;
    SupWs w;
    w.mb = ws_.take<float>((size_t)B * 4);
    w.gmax = ws_.take<float>((size_t)B * 4);
    w.gexp = ws_.take<int>(4);
    w.gpack = ws_.take<half8>((size_t)p.n_qtiles * BQ * T * 4);
    // (the weights' partial sums are laid out whether or not glogw is asked for: the size depends on the shape alone)
    w.glp = ws_.take<float>((size_t)p.nchunks * p.nslabs * 2 * npad * 4);
    w.pmp = ws_.take<float>((size_t)p.nchunks * npad * 4);
    w.part = ws_.take<float>(want_gvalues && p.nchunks > 1 ? (size_t)p.nchunks * N * T * 4 : 0);
    if (ws) *ws = w;
    return ws_.off;
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
    const int64_t npack = sup_pack_threads(p, c.T), total4 = c.N * c.T / 4;
    if (wgs > 0x7fffffffLL || (npack + 255) / 256 > 0x7fffffffLL || (total4 + 255) / 256 > 0x7fffffffLL) return NW_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(nw_bwd_values_support_prologue_kernel, dim3((unsigned)c.B), dim3(256), 0, st, c.out, c.gout, ws.mb, ws.gmax,
                       c.T);
    launch_sup_pack(c.gout, ws.gmax, ws.gexp, ws.gpack, c.B, c.T, p, st);
    float* gv_out = c.gvalues ? (p.nchunks > 1 ? ws.part : c.gvalues) : nullptr;
    const SupArgs a = {c.q, c.s_split, c.s_scale, c.s_norm2, c.v_rows, c.row_lo, c.row_hi, c.lse, c.logit_scale_dev, c.row_logw,
                       gv_out, ws, c.glogw != nullptr, c.row_lo && c.exclude != 0, (int)c.B, (int)c.N, (int)c.d, (int)c.T,
                       p.n_stiles, p.n_qtiles, p.nslabs, p.nchunks, p.tpc};
    int rc = NW_ERR_UNSUPPORTED;   // (the entry admits the five kinds alone)
#define NW_KIND_CASE(K)                                                                                               \
    case K:                                                                                                           \
        rc = launch_sup_kind<nw_bwd_values_support_kernel<K, S_NCH_MAX>, nw_bwd_values_support_kernel<K, S_NCH_MIN>>( \
            a, S_LDS, p.nch, (unsigned)wgs, st);                                                                      \
        break;
    switch (c.kind) { NW_FOR_EACH_KIND(NW_KIND_CASE) }
#undef NW_KIND_CASE
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
