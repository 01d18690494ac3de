// fused_f16p12.h -- persistent split-fp16 fused forward, 256-query tiles: EIGHT multiplying waves and FOUR loader waves
// (gfx950 / MI355X only).
//
// nw_fused_f16p_kernel<8, KIND, false, 2> (fused_f16p.h) with the tile twice as tall and the multiplying waves doubled:
//   * workgroup tile 256 queries x 128 supports, 768 threads: waves 0-7 multiply 32 queries x 128 supports each (the
//     consumer wave of fused_f16p.h), waves 8-11 fill LDS.  Two multiplying waves per SIMD cover each other's stalls, the
//     epilogue issues from two waves per SIMD, there is one barrier per 96 MFMAs of a SIMD instead of per 48, and the LDS
//     fill moves 25 % fewer bytes per flop.  No multiplying wave issues an LDS-DMA;
//   * three waves per SIMD leave 168 registers per wave: 64 accumulators, 32 for the query fragments (double-buffered:
//     this stage's and the next one's) and 32 for the support fragments, a rolling window of two pairs of 16-row blocks.
//     The last pair of a stage is multiplied BEHIND the stage's barrier, in FRONT of anything else: both waves of a SIMD
//     leave the barrier together, and a head of address arithmetic and LDS reads left the matrix pipe idle for ~180 cycles
//     per stage.  Every LDS read of the loop is issued singly behind an MFMA, at least eleven MFMAs ahead of its first
//     use, and the lane addresses are kept in bytes and moved from ring slot to ring slot under MFMAs (run_stage);
//   * 48 KB stages in a ring of three: during stage k the consumers read buffer k only, stage k+1 has landed at barrier
//     k-1, and the loaders issue stage k+2 right behind barrier k-1 into the buffer that barrier released (every read of
//     it was waited for in front of the barrier), waiting for all but the youngest stage;
//   * the same arithmetic, element for element: per accumulator the products al x bh, ah x bl, ah x bh of a stage in this
//     order, k chunks rotated by the support tile, support tiles of 128 rows, workspace layout and run tables unchanged.
//   * tile turnaround: a tile's first eight fragment reads are issued from the previous tile's epilogue, in front of its
//     partial stores, so a tile opens with MFMAs; the per-support-row score factors are made once per tile by a loader wave
//     (persistent_loader, FKIND) and read by the epilogue one 16-row block ahead of the block being scored.
// Configuration interface, tile order and loader role: persistent_pipe.h, shared with fused_f16p.h.
// Requires d / 32 >= 3 (the header of a tile rides with its first stage, two stages ahead).
//
// HALF = true (nw_fwd_opts.operand_form = 1): q and s are PLAIN fp16 rows (nw_pack_rows_f16) and `d` is their row stride
// in floats, half the embedding width.  Nothing but the multiply step differs: a 128-byte stage row is then 64
// consecutive k instead of [32 h | 32 l], the same two 16-byte slots per lane are k 8g .. 8g + 7 and 32 + 8g .. 32 + 8g + 7,
// and an accumulator takes two products per stage (k ascending) where the split form takes three for half the k.
//
// CAND = true (nw_knn_f16; HALF only): the candidate output of fused_impl.h (CandOut) instead of softmax partials.  The
// main loop, the loader role and the tile order are the same; the epilogue forms the scores as ever and then every wave
// selects, for each of its two query blocks in turn, the tile's best k scores per query (tile_candidates: 32 key registers
// per block, in the place of the dead accumulators).  No labels, run tables, statistics or partials are read or written:
// ws_runid / ws_nrun / ws_bnd / ws_num are null, ws_m / ws_den carry CandOut's key / row arrays and `k` its k.
#pragma once
#include "fused_f16p.h"

namespace nw {
namespace {

struct P12 : PipeCfg<128, 256, 8, 4, 3> {
    static constexpr int RS = BS / 16, QB = BQP / (16 * NCW);
    static constexpr int FAC_F = NHB * NH;  // the kernel's static LDS: one array of row factors (Base) per header buffer
    static_assert(LDS_BYTES + FAC_F * 4 <= 160 * 1024, "LDS of one CU");
};

// epilogue_p<8, KIND, 2, 8> (fused_f16p.h) for a wave that has 168 registers: the same operations on the same values, but
// the support factors are made per 16-row block and the scores of both query blocks are formed while the accumulators
// die, so that never more than 64 accumulator / score registers and one block's factors are live together.
// late(): called once, in front of the partial stores (CAND: behind the selection), where the score registers are dead.
template <int KIND, bool CAND = false, class Late>
__device__ __forceinline__ void epilogue_p12(f32x4 (&acc)[P12::QB][P12::RS], const float* hdr, const float* fac, int nrun, int2 bnd,
                                             float scale, float* __restrict__ ws_m,
                                             float* __restrict__ ws_den, float* __restrict__ ws_num, int B, int N,
                                             int q0, int s0, int st, int wave, int lane, int n_stiles, int k,
                                             Late&& late
#ifdef NW_DIAG_FUSED
                                             , unsigned long long (&diag_)[8], unsigned long long& last_
#endif
                                             ) {
    using P = P12;
    constexpr int RS = P::RS, QB = P::QB, BS = P::BS;
    constexpr bool NEED_NORM = (KIND != NW_SCORE_DOT);
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    const float* sn2 = hdr;
    const float* ssc = hdr + P::NH;
    const int* runid = reinterpret_cast<const int*>(hdr + 2 * P::NH);
    const float* qn2 = hdr + 3 * P::NH;
    const float* qsc_s = qn2 + P::BQP;
    const int i = lane & 15, g = lane >> 4;
    using SF = ScoreFactors<KIND>;
    float Cq[QB], Bq[QB];
#pragma unroll
    for (int j = 0; j < QB; ++j) {
        const int qrow = 16 * (QB * wave + j) + i;
        SF::query(NEED_NORM ? qn2[qrow] : 0.f, qsc_s[qrow], scale, Cq[j], Bq[j]);
    }
    NW_PSTAMP(1);
    float sc[QB][RS][4];
    // Split and half forms: the row factors come from LDS, made once per tile by a loader wave (persistent_loader, FKIND):
    // ssc holds K, sn2 Base's norm term t, the factor array Base = t * L2E^2.  The distance kinds read them one block ahead,
    // so that a block's arithmetic covers the next block's reads (the other kinds' split form spills at 168 registers with
    // the look-ahead: they read each block's K in front of its arithmetic).
    struct Fac { float4 K, t, P; };
    auto factors = [&](int r) {
        const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
        Fac f;
        f.K = *reinterpret_cast<const float4*>(ssc + 16 * r + 4 * g);
        f.t = SF::DIST ? *reinterpret_cast<const float4*>(sn2 + 16 * r + 4 * g) : zero;
        f.P = SF::DIST ? *reinterpret_cast<const float4*>(fac + 16 * r + 4 * g) : zero;
        return f;
    };
    constexpr bool AHEAD = SF::DIST;
    Fac nxt = {};
    if constexpr (!CAND && AHEAD) nxt = factors(0);
#pragma unroll
    for (int r = 0; r < RS; ++r) {
        if constexpr (!CAND) {
            constexpr float L2E2 = SF::L2E * SF::L2E;
            const Fac cur = AHEAD ? nxt : factors(r);
            if (AHEAD && r + 1 < RS) nxt = factors(r + 1);
#pragma unroll
            for (int j = 0; j < QB; ++j) {  // x = acc * (K * Cq) + (Base + Bq): three packed fp32 ops per pair
                const f32x2 cq = {Cq[j], Cq[j]}, bq = {Bq[j], Bq[j]}, l2 = {L2E2, L2E2};
                // Base + Bq bit for bit as epilogue_p is compiled (see B4r below): one fma from t for the wave's FIRST query
                // block, the rounded product plus Bq for the second
                f32x2 a01 = {0.f, 0.f}, a23 = {0.f, 0.f};
                if (SF::DIST) {
                    a01 = (j == 0) ? __builtin_elementwise_fma(f32x2{cur.t.x, cur.t.y}, l2, bq) : f32x2{cur.P.x, cur.P.y} + bq;
                    a23 = (j == 0) ? __builtin_elementwise_fma(f32x2{cur.t.z, cur.t.w}, l2, bq) : f32x2{cur.P.z, cur.P.w} + bq;
                }
                const f32x2 d01 = __builtin_elementwise_fma(f32x2{acc[j][r][0], acc[j][r][1]}, f32x2{cur.K.x, cur.K.y} * cq, a01);
                const f32x2 d23 = __builtin_elementwise_fma(f32x2{acc[j][r][2], acc[j][r][3]}, f32x2{cur.K.z, cur.K.w} * cq, a23);
                sc[j][r][0] = SF::finish_abs(d01.x);
                sc[j][r][1] = SF::finish_abs(d01.y);
                sc[j][r][2] = SF::finish_abs(d23.x);
                sc[j][r][3] = SF::finish_abs(d23.y);
                asm volatile("" : "+v"(sc[j][r][0]), "+v"(sc[j][r][1]), "+v"(sc[j][r][2]), "+v"(sc[j][r][3]));  // as below
            }
            __builtin_amdgcn_sched_barrier(0);
            continue;
        }
        // candidate form: the header as the DMAs left it, the factors made here
        const float4 n4 = NEED_NORM ? *reinterpret_cast<const float4*>(sn2 + 16 * r + 4 * g) : make_float4(0.f, 0.f, 0.f, 0.f);
        const float4 s4 = *reinterpret_cast<const float4*>(ssc + 16 * r + 4 * g);
        float4 K4, B4;
        SF::support(n4.x, s4.x, K4.x, B4.x);
        SF::support(n4.y, s4.y, K4.y, B4.y);
        SF::support(n4.z, s4.z, K4.z, B4.z);
        SF::support(n4.w, s4.w, K4.w, B4.w);
        // Bit for bit as epilogue_p is compiled: there hipcc contracts Base's last product with "+ Bq" into one fma for the
        // wave's FIRST query block (the factors are made in its basic block) and adds the rounded product for the second one
        float4 B4r = B4;
        asm volatile("" : "+v"(B4r.x), "+v"(B4r.y), "+v"(B4r.z), "+v"(B4r.w));
#pragma unroll
        for (int j = 0; j < QB; ++j) {  // x = acc * (K * Cq) + (Base + Bq): three packed fp32 ops per pair
            const f32x2 cq = {Cq[j], Cq[j]}, bq = {Bq[j], Bq[j]};
            const float4 Bj = (j == 0) ? B4 : B4r;
            const f32x2 d01 = __builtin_elementwise_fma(f32x2{acc[j][r][0], acc[j][r][1]}, f32x2{K4.x, K4.y} * cq,
                                                        f32x2{Bj.x, Bj.y} + bq);
            const f32x2 d23 = __builtin_elementwise_fma(f32x2{acc[j][r][2], acc[j][r][3]}, f32x2{K4.z, K4.w} * cq,
                                                        f32x2{Bj.z, Bj.w} + bq);
            // distance kernels: sc = +distance (u = -sc), extremum = minimum; the others: sc = u, maximum
            sc[j][r][0] = SF::finish_abs(d01.x);
            sc[j][r][1] = SF::finish_abs(d01.y);
            sc[j][r][2] = SF::finish_abs(d23.x);
            sc[j][r][3] = SF::finish_abs(d23.y);
            // made HERE, in the place of the accumulators they are made of (hipcc otherwise sinks the second query block's
            // scores behind the first one's run sums and keeps its accumulators and every block's factors until then)
            asm volatile("" : "+v"(sc[j][r][0]), "+v"(sc[j][r][1]), "+v"(sc[j][r][2]), "+v"(sc[j][r][3]));
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    NW_PSTAMP(2);
    if constexpr (CAND) {
        // One query block after the other: a block's selection holds its 32 keys next to the other block's 32 scores.  The
        // distance kinds carry +distance here; tile_candidates takes the score in base-2 units, converts it to the
        // natural-unit float, keys that very float and gives the rows past the bank the key 0.
        int ln = lane;  // made per tile: hoisted out of the tile loop, the row offsets and output indices cost the main loop registers
        asm volatile("" : "+v"(ln));
        const int ci = ln & 15, cg = ln >> 4;
#pragma unroll
        for (int j = 0; j < QB; ++j) {
            float u[RS][4];
#pragma unroll
            for (int r = 0; r < RS; ++r)
#pragma unroll
                for (int e = 0; e < 4; ++e) u[r][e] = SF::DIST ? -sc[j][r][e] : sc[j][r][e];
            tile_candidates<RS>(u, reinterpret_cast<unsigned*>(ws_m), reinterpret_cast<int*>(ws_den), B, N,
                                q0 + 16 * (QB * wave + j) + ci, s0, cg, st, n_stiles, k);
            __builtin_amdgcn_sched_barrier(0);
        }
        late();
        return;
    }
    // Both query blocks go through every phase together (extrema, lane-group reductions, exp2, run sums, reductions): the
    // swaps of one block lie under the other's hazard padding.  Each value's own operation order is that of epilogue_p.
    constexpr float WORST = SF::DIST ? INFINITY : -INFINITY;
    if (s0 + BS > N) {  // only the last support tile has rows past the bank
        const int lim = N - s0 - 4 * g;  // rows of the bank left from this lane group's first row on
#pragma unroll
        for (int j = 0; j < QB; ++j)
#pragma unroll
            for (int r = 0; r < RS; ++r)
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (16 * r + e >= lim) sc[j][r][e] = WORST;
    }
    // tile-local extremum: four independent chains per block, then the wave's four lane groups.  Minimum and maximum are
    // exact, so any grouping gives epilogue_p's bits: three-input steps (v_min3 / v_max3_f32), eight values in four of them.
    auto best = [](float a, float b) { return SF::DIST ? fminf(a, b) : fmaxf(a, b); };
    auto best3 = [&](float a, float b, float c) { return best(best(a, b), c); };
    static_assert(RS == 8, "chain k takes the 16-row blocks k and k + 4");
    float ext[QB];
#pragma unroll
    for (int j = 0; j < QB; ++j) {
        float mx[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) mx[k] = best3(sc[j][k][0], sc[j][k][1], sc[j][k][2]);
#pragma unroll
        for (int k = 0; k < 4; ++k) mx[k] = best3(mx[k], sc[j][k][3], sc[j][k + 4][0]);
#pragma unroll
        for (int k = 0; k < 4; ++k) mx[k] = best3(mx[k], sc[j][k + 4][1], sc[j][k + 4][2]);
#pragma unroll
        for (int k = 0; k < 4; ++k) mx[k] = best(mx[k], sc[j][k + 4][3]);
        ext[j] = best(best3(mx[0], mx[1], mx[2]), mx[3]);
    }
    group4_each(ext, best);
    float mloc[QB], dloc[QB], s0v[QB], s1v[QB] = {0.f, 0.f}, s2v[QB] = {0.f, 0.f};
#pragma unroll
    for (int j = 0; j < QB; ++j) {
        mloc[j] = SF::DIST ? -ext[j] : ext[j];  // the tile maximum of u
#pragma unroll
        for (int r = 0; r < RS; ++r)
#pragma unroll
            for (int e = 0; e < 4; ++e)  // 2^(u - max); 2^-inf = 0 for padded rows
                sc[j][r][e] = __builtin_amdgcn_exp2f(SF::DIST ? ext[j] - sc[j][r][e] : sc[j][r][e] - ext[j]);
    }
    NW_PSTAMP(3);
    // ---- run sums: as epilogue_p (whole 16-row blocks with a scalar 0 / 1 weight, the blocks a run boundary cuts
    // per element; more than three runs through the indicator MFMAs)
    auto add = [](float a, float b) { return a + b; };
    if (nrun <= 3) {
        float S0[QB][2] = {{0.f, 0.f}, {0.f, 0.f}}, S1[QB][2] = {{0.f, 0.f}, {0.f, 0.f}}, S2[QB][2] = {{0.f, 0.f}, {0.f, 0.f}};
        if (nrun == 1) {
#pragma unroll
            for (int r = 0; r < RS; ++r)
#pragma unroll
                for (int j = 0; j < QB; ++j) S0[j][r & 1] += (sc[j][r][0] + sc[j][r][1]) + (sc[j][r][2] + sc[j][r][3]);
        } else {
            const int b1 = bnd.x, b2 = (nrun == 3) ? bnd.y : BS;
            const float L1 = (float)(b1 - 4 * g);
            const float M2 = 1.f - (float)(b2 - 4 * g);
#pragma unroll
            for (int r = 0; r < RS; ++r) {
                const int lo = 16 * r, hi = 16 * r + 16;
                const bool in0 = hi <= b1, in2 = lo >= b2, in1 = lo >= b1 && hi <= b2;
#pragma unroll
                for (int j = 0; j < QB; ++j) {
                    const float quad = (sc[j][r][0] + sc[j][r][1]) + (sc[j][r][2] + sc[j][r][3]);
                    S0[j][r & 1] = __builtin_fmaf(in0 ? 1.f : 0.f, quad, S0[j][r & 1]);
                    S1[j][r & 1] = __builtin_fmaf(in1 ? 1.f : 0.f, quad, S1[j][r & 1]);
                    S2[j][r & 1] = __builtin_fmaf(in2 ? 1.f : 0.f, quad, S2[j][r & 1]);
                }
                if (!(in0 || in1 || in2)) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float c = (float)(16 * r + e);
                        const float w1 = __builtin_amdgcn_fmed3f(L1 - c, 0.f, 1.f);  // [t <  b1]
                        const float u2 = __builtin_amdgcn_fmed3f(c + M2, 0.f, 1.f);  // [t >= b2]
#pragma unroll
                        for (int j = 0; j < QB; ++j) {
                            const float ev = sc[j][r][e];
                            S0[j][e & 1] = __builtin_fmaf(w1, ev, S0[j][e & 1]);
                            S2[j][e & 1] = __builtin_fmaf(u2, ev, S2[j][e & 1]);
                            S1[j][e & 1] = __builtin_fmaf((1.f - w1) - u2, ev, S1[j][e & 1]);  // exact 0 / 1
                        }
                    }
                }
            }
        }
        if (nrun == 1) {
            float v[QB] = {S0[0][0] + S0[0][1], S0[1][0] + S0[1][1]};
            group4_each(v, add);
            s0v[0] = v[0], s0v[1] = v[1];
        } else if (nrun == 2) {
            float v[2 * QB] = {S0[0][0] + S0[0][1], S0[1][0] + S0[1][1], S1[0][0] + S1[0][1], S1[1][0] + S1[1][1]};
            group4_each(v, add);
            s0v[0] = v[0], s0v[1] = v[1], s1v[0] = v[2], s1v[1] = v[3];
        } else {
            float v[3 * QB] = {S0[0][0] + S0[0][1], S0[1][0] + S0[1][1], S1[0][0] + S1[0][1],
                               S1[1][0] + S1[1][1], S2[0][0] + S2[0][1], S2[1][0] + S2[1][1]};
            group4_each(v, add);
            s0v[0] = v[0], s0v[1] = v[1], s1v[0] = v[2], s1v[1] = v[3], s2v[0] = v[4], s2v[1] = v[5];
        }
#pragma unroll
        for (int j = 0; j < QB; ++j) dloc[j] = (s0v[j] + s1v[j]) + s2v[j];
    } else {
#pragma unroll
        for (int j = 0; j < QB; ++j) {
            float dl[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int r = 0; r < RS; ++r) dl[r & 3] += (sc[j][r][0] + sc[j][r][1]) + (sc[j][r][2] + sc[j][r][3]);
            dloc[j] = (dl[0] + dl[1]) + (dl[2] + dl[3]);
        }
        group4_each(dloc, add);
        // run sums on the matrix cores: indicator (A operand) x E (already in B-operand layout)
#pragma unroll
        for (int j = 0; j < QB; ++j) {
            const int b = q0 + 16 * (QB * wave + j) + i;
            for (int run_base = 0; run_base < nrun; run_base += 16) {
                f32x4 Pm = {0.f, 0.f, 0.f, 0.f};
                const int want = run_base + i;
#pragma unroll
                for (int r = 0; r < RS; ++r) {
                    const int4 rid = *reinterpret_cast<const int4*>(runid + 16 * r + 4 * g);
                    Pm = __builtin_amdgcn_mfma_f32_16x16x4f32(rid.x == want ? 1.f : 0.f, sc[j][r][0], Pm, 0, 0, 0);
                    Pm = __builtin_amdgcn_mfma_f32_16x16x4f32(rid.y == want ? 1.f : 0.f, sc[j][r][1], Pm, 0, 0, 0);
                    Pm = __builtin_amdgcn_mfma_f32_16x16x4f32(rid.z == want ? 1.f : 0.f, sc[j][r][2], Pm, 0, 0, 0);
                    Pm = __builtin_amdgcn_mfma_f32_16x16x4f32(rid.w == want ? 1.f : 0.f, sc[j][r][3], Pm, 0, 0, 0);
                }
                if (b < B) {
#pragma unroll
                    for (int jj = 0; jj < 4; ++jj) {
                        const int run = run_base + 4 * g + jj;
                        if (run < nrun) ws_num[((size_t)st * BS + run) * B + b] = Pm[jj];
                    }
                }
            }
        }
    }
    NW_PSTAMP(4);
    // ---- partial stores.  After group4_* the four lane groups of a wave hold the same bits (both halves of a swap add /
    // compare the same two operands), and the wave's two query blocks are 32 consecutive b: lane group g carries block
    // g & 1 of array g >> 1, so one full-wave store writes two 128-byte segments where 16-lane stores wrote four of 64.
    static_assert(QB == 2, "lane groups 0 / 1 carry query blocks 0 / 1, groups 2 / 3 the same blocks of the next array");
    late();
    int ln = lane;  // made per tile: hoisted out of the tile loop, the selected pointers and offsets cost the main loop registers
    asm volatile("" : "+v"(ln));
    const int b = q0 + 16 * QB * wave + (ln & 31);
    const bool blk1 = ln & 16, arr1 = ln & 32;
    const size_t tb = (size_t)st * B + b, nb = (size_t)st * BS * B + b;  // in ws_m / ws_den, in ws_num (run 0)
    if (b < B) {
        const float mv = blk1 ? mloc[1] : mloc[0], dv = blk1 ? dloc[1] : dloc[0];
        (arr1 ? ws_den : ws_m)[tb] = arr1 ? dv : mv;
        if (nrun <= 3) {  // run sums 0 and 1 in one store, the third run's from half a wave
            const float n0 = blk1 ? s0v[1] : s0v[0], n1 = blk1 ? s1v[1] : s1v[0], n2 = blk1 ? s2v[1] : s2v[0];
            if (!arr1 || nrun >= 2) ws_num[nb + (arr1 ? B : 0)] = arr1 ? n1 : n0;
            if (!arr1 && nrun == 3) ws_num[nb + 2 * (size_t)B] = n2;
        }
    }
    NW_PSTAMP(5);
}

template <int KIND, bool HALF = false, bool CAND = false>
__global__ __launch_bounds__(P12::THREADS, 3) void nw_fused_f16p_kernel_w12(
    const float* __restrict__ q, const float* __restrict__ s, const float* __restrict__ s_norm2,
    const float* __restrict__ s_scale, const float* __restrict__ q_norm2, const float* __restrict__ q_scale,
    const float* __restrict__ logit_scale, const int* __restrict__ ws_runid, const int* __restrict__ ws_nrun,
    const int* __restrict__ ws_bnd, float* __restrict__ ws_m, float* __restrict__ ws_den, float* __restrict__ ws_num, int B,
    int N, int d, int n_stiles, int n_qtiles, int qg, int k) {
    static_assert(!CAND || HALF, "the candidate form exists for half-precision rows only");
    using P = P12;
    constexpr int RS = P::RS, QB = P::QB, BS = P::BS, BQP = P::BQP, NB = P::NB;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    // Base of the tile's 128 support rows, by tile index mod NHB like the headers (distance kinds of the split and half forms;
    // written by loader wave 0, read by the epilogue).  Static, so the launch's dynamic LDS stays P::LDS_BYTES.
    __shared__ __attribute__((aligned(16))) float fac0[P12::FAC_F];
    float* hdr0 = reinterpret_cast<float*>(smem);  // NHB header buffers of HDR_F floats, by tile index mod NHB
    float4* stage = reinterpret_cast<float4*>(smem + P::HDR_BYTES);

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nk = d / BK;
    const PersistentTiles tiles(blockIdx.x, gridDim.x, n_stiles, n_qtiles, qg);  // tile order: persistent_pipe.h
    const int cu = tiles.cu, n_cu = tiles.n_cu, n_local = tiles.n_local;

    if (wave >= P::NCW) {
        persistent_loader<P, !CAND, CAND ? -1 : KIND>(tiles, wave - P::NCW, lane, hdr0, fac0, stage, q, s, s_norm2, s_scale, q_norm2, q_scale, ws_runid, B, N,
                             d);
    } else {
        // ================================ CONSUMER ================================
        const int i = lane & 15, g = lane >> 4;
        const int rsw = (i >> 1) & 7;
        const int sh = g ^ rsw, sl = (4 + g) ^ rsw;  // 16-byte slots of the high / low halves, swizzled by the row
        const int qoff = (16 * QB * wave + i) * ROW_F4, soff = (BQP + i) * ROW_F4;
        struct QF { float4 bh[QB], bl[QB]; };   // query fragments of one stage
        struct SW { float4 al[2], ah[2]; };     // support fragments of one pair of 16-row blocks
        constexpr int NW_ = RS / 2;             // pairs per stage
#ifdef NW_DIAG_FUSED
        unsigned long long diag_[8] = {0, 0, 0, 0, 0, 0, 0, 0}, last_ = 0;
#endif
#ifdef NW_DIAG_HEAD  // diagnostic build only: the ticks from a stage's barrier to its first MFMA's issue, summed in diag_[6]
        unsigned long long h0_ = 0, h1_ = 0;  // read only behind the stage's closing lgkmcnt(0)
#define NW_HEAD_STAMP(t) asm volatile("s_memtime %0" : "=s"(t))
#else
#define NW_HEAD_STAMP(t)
#endif
        auto mm = [](const float4& a, const float4& b, f32x4 c) {
            return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(half8, a), __builtin_bit_cast(half8, b), c, 0, 0, 0);
        };
        auto pin = []() { __builtin_amdgcn_sched_barrier(0); };
        f32x4 acc[QB][RS];
        // MFMA m of pair p, in the order every accumulator has always seen: four independent accumulator chains, per
        // accumulator al x bh, ah x bl, ah x bh (HALF: lo x lo, hi x hi: slot `sh` holds k 0 .. 31 of the stage's 64, slot
        // `sl` k 32 .. 63); m = 4 * product + 2 * block of the pair + query block
        constexpr int NM = HALF ? 8 : 12;
        auto mm_1 = [&](const SW& w, const QF& f, int p, int m) {
            const int ph = m >> 2, x = (m >> 1) & 1, j = m & 1;
            const float4& a = HALF ? (ph == 0 ? w.ah[x] : w.al[x]) : (ph == 0 ? w.al[x] : w.ah[x]);
            const float4& b = HALF ? (ph == 0 ? f.bh[j] : f.bl[j]) : (ph == 1 ? f.bl[j] : f.bh[j]);
            acc[j][2 * p + x] = mm(a, b, acc[j][2 * p + x]);
        };
        // the MFMAs of pair p; behind(m) is issued right behind MFMA m, in this order
        auto mm_w = [&](const SW& w, const QF& f, int p, auto&& behind) {
#pragma unroll
            for (int m = 0; m < NM; ++m) {
                mm_1(w, f, p, m);
                behind(m);
            }
            pin();
        };
        auto nothing = [](int) {};
        // The four lane addresses of the stage being read, in bytes of LDS (high / low slot of the wave's first query row
        // and of the first support row): shifted once, moved on to the next ring slot under the last MFMAs of each stage.
        typedef const __attribute__((address_space(3))) f32x4 lds_f4;
        const unsigned ring0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)(char*)stage;
        unsigned a_qh = ring0 + 16u * (qoff + sh), a_ql = ring0 + 16u * (qoff + sl);
        unsigned a_sh = ring0 + 16u * (soff + sh), a_sl = ring0 + 16u * (soff + sl);
        asm volatile("" : "+v"(a_qh), "+v"(a_ql), "+v"(a_sh), "+v"(a_sl));
        auto lds_rd = [](unsigned a, int f4) { return __builtin_bit_cast(float4, *(lds_f4*)(uintptr_t)(a + 16u * f4)); };
        auto q_h = [&](int j) { return lds_rd(a_qh, 16 * j * ROW_F4); };
        auto q_l = [&](int j) { return lds_rd(a_ql, 16 * j * ROW_F4); };
        auto s_h = [&](int blk) { return lds_rd(a_sh, 16 * blk * ROW_F4); };
        auto s_l = [&](int blk) { return lds_rd(a_sl, 16 * blk * ROW_F4); };
        auto advance = [&](int slot, int m) {  // one address per call, m = 0 .. 3
            const unsigned step = (slot + 1 == NB) ? 0u - (unsigned)((NB - 1) * P::TILE_F4 * 16) : (unsigned)(P::TILE_F4 * 16);
            unsigned& a = (m == 0) ? a_qh : (m == 1) ? a_ql : (m == 2) ? a_sh : a_sl;
            a += step;
            asm volatile("" : "+v"(a));
        };
        SW wa, wb;
        // Read n of a stage's first eight (this stage's query fragments and pair 0), in the order pair 0's MFMAs take them
        auto rd_first = [&](QF& f, SW& w, int n) {
            const bool qlo = n >= 4, slo = (n < 4) != HALF;  // the first product's operands, then the second one's
            const int r = n & 3;                             // support block 0, query blocks 0 and 1, support block 1
            if (r == 0 || r == 3) {
                const int x = r == 3;
                if (slo) w.al[x] = s_l(x);
                else w.ah[x] = s_h(x);
            } else {
                if (qlo) f.bl[r - 1] = q_l(r - 1);
                else f.bh[r - 1] = q_h(r - 1);
            }
        };
        // Read n of pair p's four, in the order the pair's MFMAs take them
        auto rd_pair = [&](SW& w, int p, int n) {
            const int x = n & 1;
            if ((n < 2) != HALF) w.al[x] = s_l(2 * p + x);
            else w.ah[x] = s_h(2 * p + x);
        };
        // One stage.  fp = the previous stage's query fragments, fc = this stage's (read here).  The last pair of the
        // previous stage (in wb) is multiplied right behind the barrier: its operands are in registers, so the matrix pipe
        // starts at once for both waves of a SIMD, and this stage's first eight reads go out one behind each of those MFMAs
        // (a tile's first stage has no held pair: its eight reads were issued by read_ahead, below, and it starts with pair
        // 0's MFMAs).  The reads of pair p + 1 lie behind the first four
        // MFMAs of pair p, the four address updates behind MFMAs 4 .. 7 of the last pair but one, after the stage's last
        // read.  No VALU or LDS instruction stands between the barrier and the first MFMA.  This stage's last pair is
        // left in wb.
#ifdef NW_DIAG_TURN  // diagnostic build only: the ticks from the end of a tile's epilogue to the issue of the next tile's first
                     // MFMA, summed in diag_[6]
        unsigned long long t0_ = 0, t1_ = 0;
#define NW_TURN_STAMP(t) asm volatile("s_memtime %0" : "=s"(t))
#else
#define NW_TURN_STAMP(t)
#endif
        auto run_stage = [&](const QF& fp, QF& fc, int slot, auto first) {
            constexpr bool FIRST = decltype(first)::value;
#ifdef NW_ABL_NORD   // timing experiment: no fragment reads in the loop (the fragments of a tile's first stage are reused)
            constexpr bool RD = FIRST;
#else
            constexpr bool RD = true;
#endif
            if constexpr (!FIRST) {
                NW_HEAD_STAMP(h0_);
                mm_w(wb, fp, NW_ - 1, [&](int m) {
                    if (m == 0) NW_HEAD_STAMP(h1_);
                    if (m < 8) {
                        pin();
                        if (RD) rd_first(fc, wa, m);
                        pin();
                    }
                });
            }
#pragma unroll
            for (int p = 0; p + 1 < NW_; ++p) {
                SW& wr = (p & 1) ? wa : wb;
                mm_w((p & 1) ? wb : wa, fc, p, [&](int m) {
                    if (FIRST && p == 0 && m == 0) NW_TURN_STAMP(t1_);
                    if (m < 4) {
                        pin();
                        if (RD) rd_pair(wr, p + 1, m);
                        pin();
                    } else if (p + 2 == NW_ && m < 8) {
                        pin();
                        advance(slot, m - 4);
                        pin();
                    }
                });
            }
            static_assert(NW_ % 2 == 0, "the last pair of a stage sits in wb");
            tile_barrier();  // every read of this stage's buffer has returned: the loaders may refill it
#ifdef NW_DIAG_HEAD
            if (!FIRST) diag_[6] += h1_ - h0_;
#endif
#ifdef NW_DIAG_TURN
            if (FIRST && t0_) diag_[6] += t1_ - t0_;
#endif
        };
        using Yes = std::integral_constant<bool, true>;
        using No = std::integral_constant<bool, false>;

        // exp(logit_scale) once per launch, in a scalar register (made per tile, hipcc parks the constants of expf in vector
        // registers across the main loop)
        float scale = 1.f;
        if (KIND == NW_SCORE_CLIP)
            scale = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, expf(*logit_scale))));
        tile_barrier();  // P
        int gi = 0;     // ring slot of the current tile's first stage
        int par = 0;     // header buffer of the current tile
        auto next_slot = [&]() {
            const int b = gi;
            gi = (gi + 1 == NB) ? 0 : gi + 1;
            return b;
        };
#ifdef NW_DIAG_FUSED
        last_ = __builtin_amdgcn_s_memtime();
        const unsigned long long first_ = last_, first_rt_ = __builtin_amdgcn_s_memrealtime();
#endif
        // A tile's first eight fragment reads (its first stage's query fragments and pair 0, into f0 and wa) are issued from
        // the previous tile's epilogue.  At that tile's last stage barrier only the youngest stage the loaders have issued may
        // still be in flight (wait_landed, persistent_pipe.h), and that is the next tile's SECOND stage: its first stage and
        // its header have landed.  The four lane addresses point at that stage's ring slot already (advance in the last
        // stage), and f0 and wa are dead in the epilogue.  A workgroup's first tile reads behind barrier P.
        QF f0, f1;
        auto read_ahead = [&]() {
#pragma unroll
            for (int n = 0; n < 8; ++n) {
                rd_first(f0, wa, n);
                pin();
            }
        };
        if (cu < n_local) read_ahead();
        for (int T = cu; T < n_local; T += n_cu) {
            const bool more = T + n_cu < n_local;  // the workgroup's last tile has no successor
            auto late = [&]() {
                pin();
                if (more) read_ahead();
                pin();
            };
            int qt, st;
            tiles.decode(T, qt, st);
            const int q0 = qt * BQP, s0 = st * BS;
            int nrun = 0;
            int2 bnd = {0, 0};
            if constexpr (!CAND) {
                nrun = ws_nrun[st];  // wave-uniform: scalar loads, used after the main loop
                bnd = *reinterpret_cast<const int2*>(ws_bnd + 2 * (size_t)st);  // first rows of runs 1 and 2
            }
#pragma unroll
            for (int j = 0; j < QB; ++j)
#pragma unroll
                for (int r = 0; r < RS; ++r) acc[j][r] = f32x4{0.f, 0.f, 0.f, 0.f};
#ifdef NW_ABL_NORD
#pragma unroll
            for (int n = 0; n < 8; ++n) rd_first(f1, wa, n);
#endif
            run_stage(f1, f0, next_slot(), Yes{});
            int kt = 1;
            for (; kt + 1 < nk; kt += 2) {
                run_stage(f0, f1, next_slot(), No{});
                run_stage(f1, f0, next_slot(), No{});
            }
            if (kt < nk) {
                run_stage(f0, f1, next_slot(), No{});
                mm_w(wb, f1, NW_ - 1, nothing);
            } else {
                mm_w(wb, f0, NW_ - 1, nothing);
            }
            NW_PSTAMP(0);
#ifndef NW_ABL_NOEPI
            epilogue_p12<KIND, CAND>(acc, hdr0 + par * P::HDR_F, fac0 + par * P::NH, nrun, bnd, scale, ws_m, ws_den, ws_num, B, N, q0, s0, st, wave,
                                     lane, n_stiles, k, late
#ifdef NW_DIAG_FUSED
                                     , diag_, last_
#endif
                                     );
#else
            keep_acc_alive(acc, ws_m, nrun, bnd);
            late();
#endif
            par = (par + 1 == P::NHB) ? 0 : par + 1;
#ifdef NW_DIAG_TURN
            asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t0_));  // carried over the loop's back edge: landed first
#endif
#if !defined(NW_DIAG_HEAD) && !defined(NW_DIAG_TURN)
            NW_PSTAMP(6);
#endif
        }
#ifdef NW_DIAG_FUSED
        diag_write_out(diag_, last_, first_, first_rt_);
#endif
    }
}

}  // namespace
}  // namespace nw
