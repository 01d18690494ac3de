// persistent_pipe.h -- what the persistent split-fp16 kernels share (nw_fused_f16p_kernel, fused_f16p.h;
// nw_fused_f16p_kernel_w12, fused_f16p12.h): the LDS / pipeline configuration, the tile order, the whole loader role
// and the tails of the diagnostic builds.  The consumer main loops and the tile epilogues are the kernels' own.
#pragma once
#include "tile_core.h"

namespace nw {
namespace {

#ifdef NW_DIAG_FUSED  // diagnostic build only (tools/bench_fused.hip): per-workgroup phase totals
__device__ unsigned long long nw_diag_p[8 * 1024];
__device__ unsigned long long nw_diag_rt[2 * 1024];   // s_memrealtime (100 MHz) at the first / last stamp of a workgroup
#define NW_PSTAMP(k)                                                                         \
    do {                                                                                     \
        unsigned long long now_;                                                             \
        __builtin_amdgcn_sched_barrier(0);                                                   \
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(now_)::"memory");         \
        __builtin_amdgcn_sched_barrier(0);                                                   \
        diag_[k] += now_ - last_;                                                            \
        last_ = now_;                                                                        \
    } while (0)

// phase totals of a workgroup (diag_[0..6], stamped by its wave 0) and its lifetime, written out by thread 0
__device__ __forceinline__ void diag_write_out(const unsigned long long (&diag_)[8], unsigned long long last_,
                                               unsigned long long first_, unsigned long long first_rt_) {
    if (threadIdx.x == 0 && blockIdx.x < 1024) {
        for (int k = 0; k < 7; ++k) nw_diag_p[8 * blockIdx.x + k] = diag_[k];
        nw_diag_p[8 * blockIdx.x + 7] = last_ - first_;
        nw_diag_rt[2 * blockIdx.x] = first_rt_;
        nw_diag_rt[2 * blockIdx.x + 1] = __builtin_amdgcn_s_memrealtime();
    }
}
#else
#define NW_PSTAMP(k)
#endif

// -DNW_ABL_NOEPI (timing experiment, tools/bench_fused.hip): in the place of a tile's epilogue, keeps every
// accumulator chain alive
template <int QB, int RS>
__device__ __forceinline__ void keep_acc_alive(const f32x4 (&acc)[QB][RS], float* ws_m, int nrun, int2 bnd) {
    f32x4 sum_ = {0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < QB; ++j)
        for (int r = 0; r < RS; ++r) sum_ += acc[j][r];
    if (sum_[0] + sum_[1] + sum_[2] + sum_[3] == 12345.678f) ws_m[threadIdx.x] = sum_[0] + nrun + bnd.x;
}

// A workgroup of NCW_ consumer (MFMA) waves and NLW_ loader waves on tiles of BQP_ queries x BS_ supports, with a ring
// of NB_ stage buffers behind NHB header buffers in LDS.
template <int BS_, int BQP_, int NCW_, int NLW_, int NB_>
struct PipeCfg {
    static constexpr int BS = BS_, BQP = BQP_, NCW = NCW_, NLW = NLW_;
    static constexpr int THREADS = 64 * (NCW + NLW);
    static constexpr int NB = NB_;                      // ring depth
    static constexpr int AHEAD = NB - 1;                // stages in flight per loader wave
    static constexpr int TILE_F4 = (BQP + BS) * ROW_F4; // one stage: 128 B per row, queries, then supports
    static constexpr int NT = (BQP + BS) / 8;           // stage DMA pieces (1 KB = 8 rows)
    static constexpr int NI = NT / NLW;                 // ... per loader wave
    static constexpr int NQI = BQP / 8 / NLW;           // of them query pieces (the first ones)
    static constexpr int N64 = (BS + 63) / 64;          // 64-row DMA pieces per support-side header array
    static constexpr int NH = N64 * 64;                 // entries per support-side array in LDS
    static constexpr int HDR_F = 3 * NH + 2 * BQP;      // sn2 | ssc | runid | qn2[BQP] | qsc[BQP]
    static constexpr int NP = 3 * N64 + 2 * (BQP / 64); // header pieces (256 B each)
    static constexpr int HPW = (NP + NLW - 1) / NLW;    // ... per loader wave
    static constexpr int NHB = 3;                       // header buffers (tile index mod 3)
    static constexpr size_t HDR_BYTES = (size_t)NHB * HDR_F * 4;
    static constexpr size_t LDS_BYTES = HDR_BYTES + (size_t)NB * TILE_F4 * 16;  // dynamic LDS of a launch
    static_assert(NT % NLW == 0, "every loader wave issues the same number of pieces");
    static_assert(BQP % (8 * NLW) == 0, "query and support pieces must not share a loader round");
    static_assert(HDR_BYTES % 16 == 0, "stage buffers must stay 16-byte aligned");
    static_assert(NI + HPW < 64, "vmcnt is a 6-bit field");
};

// ---- tile order.  Workgroup b runs on XCD b % 8 (round-robin dispatch, one workgroup per CU), and
// every XCD has its own 4 MiB L2, so each XCD walks its OWN list of tiles in an order that keeps
// its working set in that L2: XCD x owns the support tiles st = x (mod 8); its list is cut into
// groups of `qg` query tiles (kept resident: qg * BQP * 2 KB at d = 512), and inside a group runs support-tile
// major, so the n_cu workgroups of the XCD are on ~n_cu/qg support tiles x qg query tiles at any
// time.
// The support tiles beyond the last full round of 8 (n_stiles % 8 of them) are dealt by QUERY tile
// (qt = x mod 8) instead, so every XCD gets the same number of tiles to within n_stiles % 8: with 49
// support tiles (a shard of the K3 bank at 8 ranks) one XCD would otherwise walk 7 and seven XCDs 6.
// Workgroup `cu` of its XCD takes the entries cu, cu + n_cu, ... < n_local of the XCD's list.
// n / dv for 0 <= n < 2^31 and a divisor that is fixed for the launch, without the float reciprocal of hipcc's own expansion
// (a v_rcp_iflag_f32 and a v_readfirstlane in a chain of scalar instructions): rcp = floor((2^32 - 1) / dv) is made once per
// launch, and because 0 <= 2^32 / dv - rcp <= 1 the high half of n * rcp is short of n / dv by less than n / 2^32 < 1: it is
// the quotient or one below it, and one step corrects it.  A divisor of 0 (a list part that is empty, never decoded) counts as 1.
struct TileDiv {
    unsigned dv, rcp;
    __device__ __forceinline__ void set(int d) {
        dv = (unsigned)max(d, 1);
        rcp = 0xFFFFFFFFu / dv;
    }
    static __device__ __forceinline__ void divmod(unsigned n, unsigned dv, unsigned rcp, int& quo, int& rem) {
        unsigned q = __umulhi(n, rcp), r = n - q * dv;
        if (r >= dv) ++q, r -= dv;
        quo = (int)q, rem = (int)r;
    }
    __device__ __forceinline__ void divmod(int n, int& quo, int& rem) const { divmod((unsigned)n, dv, rcp, quo, rem); }
};

struct PersistentTiles {
    int xcd, cu, n_cu;
    int n_qtiles, qg;
    int ns_x;       // full rounds: support tiles st = stl * 8 + x
    int n_full;
    int n_local;    // tiles of this XCD
    TileDiv by_nq;  // nq_x: query tiles of this XCD in the leftover part
    TileDiv by_grp; // qg * ns_x: tiles of a group of query tiles
    TileDiv by_qg;  // a group's query tiles: qg, ...
    TileDiv by_last;  // ... but n_qtiles % qg in the last group when that is not 0
    __device__ __forceinline__ PersistentTiles(unsigned block, unsigned grid, int n_stiles, int n_qtiles_, int qg_)
        : xcd(block & 7), cu(block >> 3), n_cu(grid >> 3), n_qtiles(n_qtiles_), qg(qg_) {
        ns_x = n_stiles >> 3;
        n_full = ns_x * n_qtiles;
        const int rem = n_stiles & 7;  // leftover support tiles 8 * ns_x .. n_stiles - 1
        const int nq_x = (n_qtiles - xcd + 7) >> 3;
        n_local = n_full + rem * nq_x;
        by_nq.set(nq_x);
        by_grp.set(qg * ns_x);
        by_qg.set(qg);
        by_last.set(n_qtiles % max(qg, 1));
    }
    __device__ __forceinline__ void decode(int L, int& qt, int& st) const {
        if (L >= n_full) {  // leftover part, support-tile major
            int j, r;
            by_nq.divmod(L - n_full, j, r);
            st = 8 * ns_x + j;
            qt = xcd + 8 * r;
            return;
        }
        int gi, r, stl, qi;
        by_grp.divmod(L, gi, r);
        const int g = min(qg, n_qtiles - gi * qg);  // one of two values per launch: the last group may be short
        TileDiv::divmod((unsigned)r, (unsigned)g, g == qg ? by_qg.rcp : by_last.rcp, stl, qi);
        qt = gi * qg + qi;
        st = stl * 8 + xcd;
    }
};

// The loader role: loader wave lw of P::NLW keeps ONE stage pipeline running over the workgroup's tiles, P::AHEAD stages
// in flight, and DMAs each tile's header (support norms, row scales, run ids; query norms and scales) into header
// buffer (tile index mod P::NHB) together with the tile's first stage.  One tile_barrier() per stage plus one in front,
// matched by the consumers.  -DNW_ABL_NODMA (timing experiment, results wrong): the stages are not filled.
// RUNID = false (the candidate-output form, which reads no run tables: ws_runid is null): the run-id pieces repeat the row
// scales' pieces instead (same bytes to the same place), so that every stage keeps its count of DMAs.
// FKIND >= 0 (a score kind; P has the factor array): once a tile's header has landed, loader wave 0 rewrites its support side
// into the factors the tile epilogue would otherwise make in every multiplying wave and lane group
// (ScoreFactors<FKIND>::support_parts): ssc becomes K, sn2 becomes Base's norm term t, and Base = t * L2E^2 goes to
// fac0, the kernel's own NHB arrays of NH floats beside the headers (static LDS: the launch's dynamic LDS is unchanged).
template <class P, bool RUNID = true, int FKIND = -1>
__device__ __forceinline__ void persistent_loader(const PersistentTiles& tiles, int lw, int lane, float* hdr0, float* fac0, float4* stage,
                                                  const float* __restrict__ q, const float* __restrict__ s,
                                                  const float* __restrict__ s_norm2, const float* __restrict__ s_scale,
                                                  const float* __restrict__ q_norm2, const float* __restrict__ q_scale,
                                                  const int* __restrict__ ws_runid, int B, int N, int d) {
    constexpr int BS = P::BS, BQP = P::BQP, NI = P::NI, NLW = P::NLW;
    const int nk = d / BK;
    const int n_local = tiles.n_local, n_cu = tiles.n_cu;
    unsigned voff[NI];
    int iT = tiles.cu, ikt = 0, irot = 0, ipar = 0;  // issue cursor: (tile of this XCD's list, stage), header buffer
    int iq0 = 0, is0 = 0, ist = 0;
    int gs = 0;                                      // ring slot of the stage under the cursor
    auto set_tile = [&](int T) {
        int qt, st;
        tiles.decode(T, qt, st);
        iq0 = qt * BQP;
        is0 = st * BS;
        ist = st;
        irot = st % nk;
#pragma unroll
        for (int m = 0; m < NI; ++m) {
            const int R = 8 * (lw + NLW * m) + (lane >> 3);       // row of the stage image: queries, then supports
            const int lslot = (lane & 7) ^ ((R >> 1) & 7);        // swizzle on the source side (an LDS-DMA writes linearly)
            // relative to the tile's first rows (64-bit bases in issue_next): no 4 GB limit on the bank
            const int rel = (m < P::NQI) ? min(iq0 + R, B - 1) - iq0 : min(is0 + R - BQP, N - 1) - is0;
            voff[m] = ((unsigned)rel * (unsigned)d + lslot * 4) * 4u;
        }
    };
    auto dma4 = [&](const void* src, float* dst) {  // one dword per lane -> dst[lane]
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                         (__attribute__((address_space(3))) void*)dst, 4, 0, 0);
    };
    // header pieces of the tile under the issue cursor: HPW per loader wave (piece ids past the last one repeat the
    // last piece: same bytes to the same place)
    auto issue_header = [&]() {
        float* h = hdr0 + ipar * P::HDR_F;
#pragma unroll
        for (int k = 0; k < P::HPW; ++k) {
            const int pc = min(lw + NLW * k, P::NP - 1);
            if (pc < 3 * P::N64) {
                const int arr = pc / P::N64, c = pc - arr * P::N64;
                const int row = is0 + 64 * c + lane;
                float* dst = h + arr * P::NH + 64 * c;
                if (arr == 0) dma4(s_norm2 + min(row, N - 1), dst);
                else if (arr == 1) dma4(s_scale + min(row, N - 1), dst);
                else if constexpr (RUNID) dma4(ws_runid + (size_t)ist * BS + 64 * c + lane, dst);  // padded by 64 entries
                else dma4(s_scale + min(row, N - 1), h + P::NH + 64 * c);
            } else {
                const int qp = pc - 3 * P::N64, arr = qp / (BQP / 64), c = qp - arr * (BQP / 64);  // qn2 pieces, then qsc pieces
                const int row = min(iq0 + 64 * c + lane, B - 1);
                dma4((arr == 0 ? q_norm2 : q_scale) + row, h + 3 * P::NH + arr * BQP + 64 * c);
            }
        }
    };
    bool young_hdr = false;  // does the youngest issued stage carry header pieces?
    auto issue_next = [&]() {  // returns false once every stage of every tile has been issued
        if (iT >= n_local) return false;
        int kc = ikt + irot;
        if (kc >= nk) kc -= nk;
        float4* buf = stage + gs * P::TILE_F4;
        const char* qb = reinterpret_cast<const char*>(q + (size_t)iq0 * d) + (size_t)kc * BK * 4;
        const char* sb = reinterpret_cast<const char*>(s + (size_t)is0 * d) + (size_t)kc * BK * 4;
#ifndef NW_ABL_NODMA
#pragma unroll
        for (int m = 0; m < NI; ++m) {
            const char* g = ((m < P::NQI) ? qb : sb) + voff[m];
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                             (__attribute__((address_space(3))) void*)(buf + 64 * (lw + NLW * m)), 16, 0, 0);
        }
#else
        (void)qb; (void)sb; (void)buf;
#endif
        young_hdr = (ikt == 0);
        if (young_hdr) issue_header();  // after the stage's own pieces: they are waited for last
        gs = (gs + 1 == P::NB) ? 0 : gs + 1;
        if (++ikt == nk) {
            ikt = 0;
            ipar = (ipar + 1 == P::NHB) ? 0 : ipar + 1;
            iT += n_cu;
            if (iT < n_local) set_tile(iT);
        }
        return true;
    };
#ifndef NW_ABL_NODMA
    constexpr int YOUNG = NI;  // DMAs of a stage, without its header
#else
    constexpr int YOUNG = 0;
#endif
    auto wait_landed = [&](bool issued) {  // everything but the youngest stage of this wave has landed
        if (!issued) wait_vmcnt<0>();
        else if (young_hdr) wait_vmcnt<YOUNG + P::HPW>();
        else wait_vmcnt<YOUNG>();
    };
    // The header of the tile whose first stage the consumers are about to multiply landed with that stage, so it was
    // published by the barrier before (wait_landed: everything but the youngest stage).  Its readers are the tile's epilogue,
    // nk barriers later; the writes are complete at the next one (tile_barrier waits lgkmcnt(0)).  LDS is read and written
    // by hand: hipcc would put a vmcnt(0) in front of a ds_read that may alias an LDS-DMA and drain the stages in flight.
    int cpar = 0;  // header buffer of that tile
    auto make_factors = [&]() {
        if constexpr (FKIND >= 0) {
            static_assert(P::NH == 128, "two rows per lane of one wave");
            using SF = ScoreFactors<FKIND>;
            if (lw == 0) {
                const unsigned a = (unsigned)(uintptr_t)(__attribute__((address_space(3))) float*)(hdr0 + cpar * P::HDR_F) + 4u * lane;
                const unsigned af = (unsigned)(uintptr_t)(__attribute__((address_space(3))) float*)(fac0 + cpar * P::NH) + 4u * lane;
                float n2[2], sc[2];
                asm volatile("ds_read_b32 %0, %4\n\tds_read_b32 %1, %4 offset:256\n\t"
                             "ds_read_b32 %2, %4 offset:%5\n\tds_read_b32 %3, %4 offset:%6\n\ts_waitcnt lgkmcnt(0)"
                             : "=&v"(n2[0]), "=&v"(n2[1]), "=&v"(sc[0]), "=&v"(sc[1])
                             : "v"(a), "n"(4 * P::NH), "n"(4 * P::NH + 256)
                             : "memory");
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    float K, t, Bp;
                    SF::support_parts(n2[h], sc[h], K, t, Bp);
                    asm volatile("ds_write_b32 %0, %1 offset:%2" ::"v"(a), "v"(K), "n"(4 * P::NH + 256 * h) : "memory");
                    if constexpr (SF::DIST) {
                        if constexpr (SF::NORMALISED) asm volatile("ds_write_b32 %0, %1 offset:%2" ::"v"(a), "v"(t), "n"(256 * h) : "memory");
                        asm volatile("ds_write_b32 %0, %1 offset:%2" ::"v"(af), "v"(Bp), "n"(256 * h) : "memory");
                    }
                }
            }
            cpar = (cpar + 1 == P::NHB) ? 0 : cpar + 1;
        }
    };
    if (iT < n_local) set_tile(iT);
    bool more = true;
#pragma unroll
    for (int k0 = 0; k0 < P::AHEAD; ++k0) more = issue_next();
    wait_landed(more);
    tile_barrier();  // P: all but the youngest issued stage (and the first tile's header) have landed
    for (int T = tiles.cu; T < n_local; T += n_cu) {
        for (int kt = 0; kt < nk; ++kt) {
            more = issue_next();
            if (kt == 0) make_factors();
            wait_landed(more);
            tile_barrier();
        }
    }
}

}  // namespace
}  // namespace nw
