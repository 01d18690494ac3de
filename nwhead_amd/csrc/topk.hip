// topk.hip -- the k best supports of every query from a (B,N) score matrix (gfx950 / MI355X only).
//
// Replaces the full descending argsort the reference runs for its neighbour modes and then cuts to k
// columns (KNN.__call__, nwhead/utils.py:185-193; NWNet.get_neighbors, nwhead/nw.py:245-249):
//   idx[b][0..k) = the first k columns of argsort(scores[b], descending, stable)
// i.e. best score first, equal scores in ascending index order -- bit-exact, not approximate.
//
// One 1024-thread workgroup per row (four independent loads in flight per thread in the histogram passes):
//   1. radix select on the order-preserving uint image of the floats, four 8-bit digits from the top:
//      an LDS histogram of the digit among the elements that match the prefix found so far gives the
//      digit of the k-th largest; lanes of a wave that hit the same bin are merged before the LDS
//      atomic (the top byte of a score row is almost constant: one hot bin);
//   2. ordered compaction: every thread owns a CONTIGUOUS index range, counts its elements above the
//      threshold T and equal to it, a block scan turns the counts into output slots, so the ties that
//      make it are the lowest-indexed ones;
//   3. bitonic sort of the (at most 1024) survivors in LDS by (value desc, index asc).
// Rows of up to 65536 scores are read from memory ONCE and stay in registers (16 or 64 per thread); longer rows are
// re-read in every pass (five reads).
//
// MAPPED (nw_knn_f32): the row holds the CANDIDATES of the fused tile kernel's selection epilogue instead of scores --
// ordered_bits keys (0: an empty slot) with a column -> bank-row map.  Equal keys stand in ascending bank-row order along
// the row, so the same stable rule gives (score descending, bank row ascending); outputs are the mapped rows and the
// floats of the keys.
// PAD (nw_knn_window_f32): a row may hold fewer than k candidates.  Empty slots then count as elements below every score
// (the threshold can fall to 0, and "equal to the threshold" picks as many of them as are missing), and a selected key
// of 0 is emitted as row -1 and value -inf: the valid entries come first, in the usual order.
#include "nw_internal.h"

namespace nw {
namespace {

constexpr int TK_THREADS = 1024;
constexpr int TK_MAXK = 1024;

constexpr int TK_U = 8;       // independent loads in flight per thread in the histogram passes (long rows: 254 -> ... us at N = 50000 from 4)
// REGS > 0: the row is read from memory ONCE.  Wave w owns the contiguous segment [w seg, (w + 1) seg) of the row
// (seg a multiple of 64, 16 seg >= N) and keeps it in registers, element e of lane l = w seg + 64 e + l (coalesced
// loads); the histogram passes and the ordered compaction (ranks from ballots inside the wave, wave bases from one
// LDS round) all work from those registers.  REGS = 0 (N > 65536): the row is re-read in every pass.
template <int REGS, bool MAPPED = false, bool PAD = false>
__global__ __launch_bounds__(TK_THREADS) void nw_topk_kernel(const float* __restrict__ scores,
                                                             int64_t* __restrict__ idx_out,
                                                             float* __restrict__ val_out, int N, int k,
                                                             const int* __restrict__ row_map) {
    constexpr bool CACHED = REGS > 0;
    constexpr int TK_REGS = CACHED ? REGS : TK_U;
    __shared__ unsigned hist[256];
    __shared__ unsigned sel_prefix, sel_need;  // prefix of the k-th largest so far; how many of its bin are still needed
    __shared__ unsigned scan_gt[TK_THREADS / 64], scan_eq[TK_THREADS / 64];
    __shared__ unsigned cand_u[TK_MAXK];
    __shared__ int cand_i[TK_MAXK];
    const int tid = threadIdx.x, lane = tid & 63;
    const float* row = scores + (size_t)blockIdx.x * N;
    auto key_at = [&](int i) { return MAPPED ? reinterpret_cast<const unsigned*>(row)[i] : ordered_bits(row[i]); };
    auto emit = [&](int slot, int ix, unsigned u) {   // u: the element's key (read by PAD only)
        if (PAD && u == 0u) {
            idx_out[(size_t)blockIdx.x * k + slot] = -1;
            if (val_out) val_out[(size_t)blockIdx.x * k + slot] = -INFINITY;
        } else if (MAPPED) {
            idx_out[(size_t)blockIdx.x * k + slot] = row_map[(size_t)blockIdx.x * N + ix];
            if (val_out) val_out[(size_t)blockIdx.x * k + slot] = ordered_bits_to_float(key_at(ix));
        } else {
            idx_out[(size_t)blockIdx.x * k + slot] = ix;
            if (val_out) val_out[(size_t)blockIdx.x * k + slot] = row[ix];
        }
    };

    // ---- 1. radix select of the k-th largest
    if (tid == 0) {
        sel_prefix = 0;
        sel_need = (unsigned)k;
    }
    unsigned ureg[TK_REGS];   // CACHED: element wave * seg + 64 e + lane of the row
    const int wv = tid >> 6;
    const int seg = ((N + 16 * 64 - 1) / (16 * 64)) * 64;   // elements per wave
    if (CACHED) {
#pragma unroll
        for (int e = 0; e < TK_REGS; ++e) {   // coalesced, independent loads; the only pass over memory
            const int i = wv * seg + 64 * e + lane;
            ureg[e] = (64 * e < seg && i < N) ? key_at(i) : 0u;
        }
    }
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        if (tid < 256) hist[tid] = 0;
        __syncthreads();
        const unsigned prefix = sel_prefix;
        // one element into the histogram: lanes that hit the same bin are merged first (two rounds take care of a hot bin),
        // then plain atomics; only the top byte (sign + high exponent bits) is that concentrated -- the lower digits are
        // spread over the bins and the merge would cost more than the atomics it saves
        auto count = [&](unsigned u, bool ok) {
            bool live = ok && ((pass == 0) || ((u >> (shift + 8)) == (prefix >> (shift + 8))));
            const unsigned bin = (u >> shift) & 255u;
            for (int round = 0; round < (pass == 0 ? 2 : 0); ++round) {
                const unsigned long long act = __ballot(live);
                if (!act) break;
                const unsigned b0 = __builtin_amdgcn_readlane(bin, __builtin_ctzll(act));
                const unsigned long long same = __ballot(live && bin == b0);
                if (live && bin == b0) {
                    if (lane == __builtin_ctzll(same)) atomicAdd(&hist[b0], (unsigned)__builtin_popcountll(same));
                    live = false;
                }
            }
            if (live) atomicAdd(&hist[bin], 1u);
        };
        if (CACHED) {
#pragma unroll
            for (int e = 0; e < TK_REGS; ++e) {
                // (PAD: the row's empty slots count too, so that the k-th largest always exists)
                count(ureg[e], PAD ? (64 * e < seg && wv * seg + 64 * e + lane < N) : ureg[e] != 0u);   // 0 is the image of no float (the smallest, -inf, is 0x007fffff): "not an element"
                __builtin_amdgcn_sched_barrier(0);   // (one element at a time: hoisted ballots spill the scalar file)
            }
        } else {
            for (int i0 = 0; i0 < N; i0 += TK_U * TK_THREADS) {
                unsigned u4[TK_U];
                bool ok[TK_U];
#pragma unroll
                for (int e = 0; e < TK_U; ++e) {  // coalesced, independent: TK_U loads in flight
                    const int i = i0 + e * TK_THREADS + tid;
                    ok[e] = i < N;
                    u4[e] = ok[e] ? key_at(i) : 0u;
                }
#pragma unroll
                for (int e = 0; e < TK_U; ++e) count(u4[e], ok[e]);
            }
        }
        __syncthreads();
        if (tid < 64) {  // one wave walks the 256 bins from the top: 4 bins per lane
            unsigned c[4], tot = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                c[j] = hist[255 - (4 * tid + j)];
                tot += c[j];
            }
            unsigned incl = tot;  // inclusive scan over lanes (lane 0 = top bins)
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const unsigned v = __shfl_up(incl, o);
                if (lane >= o) incl += v;
            }
            unsigned before = incl - tot;  // elements in bins above this lane's four
            const unsigned need = sel_need;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (before < need && before + c[j] >= need) {  // exactly one (lane, j) satisfies this
                    sel_prefix = prefix | ((unsigned)(255 - (4 * tid + j)) << shift);
                    sel_need = need - before;
                }
                before += c[j];
            }
        }
        __syncthreads();
    }
    const unsigned T = sel_prefix;       // ordered bits of the k-th largest element
    const unsigned n_eq = sel_need;      // how many elements equal to T make it (the lowest-indexed ones)
    const unsigned n_gt = (unsigned)k - n_eq;

    // ---- 2. ordered compaction (ties: the lowest indices make it)
    if (CACHED) {
        // from the registers: every wave counts its segment, one LDS round gives the waves' bases, then the wave walks
        // its elements in index order and ranks the survivors of each 64 with ballots
        unsigned cg = 0, ce = 0;
#pragma unroll
        for (int e = 0; e < TK_REGS; ++e) {
            // (register slots past the wave's segment or the row hold 0, below every image: with T > 0 they are below T
            //  and drop out by themselves.  PAD with T = 0 -- fewer than k candidates -- ranks them among the row's own
            //  empty slots as "equal to T", and some of the n_eq places can go to them, with an index i that is past the
            //  row or inside the next wave's segment: harmless, because nothing is read through that index -- emit writes
            //  (-1, -inf) for EVERY key of 0 whatever its index, the histogram passes counted the row's own empty slots
            //  only, so n_gt + n_eq = k slots are filled all the same, and every element above T, the valid ones, keeps
            //  its place)
            cg += (unsigned)__builtin_popcountll(__ballot(ureg[e] > T));
            ce += (unsigned)__builtin_popcountll(__ballot(ureg[e] == T));
            __builtin_amdgcn_sched_barrier(0);   // (one ballot pair at a time: hoisted together they spill the scalar file)
        }
        if (lane == 0) {
            scan_gt[wv] = cg;
            scan_eq[wv] = ce;
        }
        __syncthreads();
        unsigned og = 0, oe = 0;
        for (int w = 0; w < wv; ++w) {
            og += scan_gt[w];
            oe += scan_eq[w];
        }
        const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
        for (int e = 0; e < TK_REGS; ++e) {
            const int i = wv * seg + 64 * e + lane;
            const bool isg = ureg[e] > T, ise = ureg[e] == T;
            const unsigned long long mg = __ballot(isg), me = __ballot(ise);
            if (isg) {
                const unsigned slot = og + (unsigned)__builtin_popcountll(mg & below);
                cand_u[slot] = ureg[e];
                cand_i[slot] = i;
            } else if (ise) {
                const unsigned slot = oe + (unsigned)__builtin_popcountll(me & below);
                if (slot < n_eq) {
                    cand_u[n_gt + slot] = ureg[e];
                    cand_i[n_gt + slot] = i;
                }
            }
            og += (unsigned)__builtin_popcountll(mg);
            oe += (unsigned)__builtin_popcountll(me);
            __builtin_amdgcn_sched_barrier(0);
        }
    } else {
    // contiguous per-thread index ranges, the row read twice more
    const int per = (N + TK_THREADS - 1) / TK_THREADS;
    const int lo = min(tid * per, N), hi = min(lo + per, N);
    unsigned cg = 0, ce = 0;
    for (int i = lo; i < hi; ++i) {
        const unsigned u = key_at(i);
        cg += u > T;
        ce += u == T;
    }
    // exclusive block scans of the two counts: inside a wave by shuffles, across the 16 waves through LDS (two
    // barriers; a Hillis-Steele scan over the 1024 threads took twenty)
    unsigned ig = cg, ie = ce;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned a = __shfl_up(ig, o), b = __shfl_up(ie, o);
        if (lane >= o) {
            ig += a;
            ie += b;
        }
    }
    if (lane == 63) {
        scan_gt[wv] = ig;
        scan_eq[wv] = ie;
    }
    __syncthreads();
    unsigned og = ig - cg, oe = ie - ce;
    for (int w = 0; w < wv; ++w) {
        og += scan_gt[w];
        oe += scan_eq[w];
    }
    for (int i = lo; i < hi; ++i) {
        const unsigned u = key_at(i);
        if (u > T) {
            cand_u[og] = u;
            cand_i[og] = i;
            ++og;
        } else if (u == T) {
            if (oe < n_eq) {
                cand_u[n_gt + oe] = u;
                cand_i[n_gt + oe] = i;
            }
            ++oe;
        }
    }
    }
    __syncthreads();

    // ---- 3. bitonic sort of the k survivors: value descending, index ascending
    int P = 1;
    while (P < k) P <<= 1;
    for (int x = k + tid; x < P; x += TK_THREADS) {  // padding sorts last
        cand_u[x] = 0;
        cand_i[x] = 0x7fffffff;
    }
    __syncthreads();
    auto before = [](unsigned ua, int ia, unsigned ub, int ib) { return ua > ub || (ua == ub && ia < ib); };
    if (P <= 64) {
        // up to 64 survivors: one wave sorts them in registers (a bitonic network of shuffles, no barriers; the LDS
        // version below costs a block-wide barrier per stage, ten of them at k = 10)
        if (tid < 64) {
            unsigned u = tid < P ? cand_u[tid] : 0u;
            int ix = tid < P ? cand_i[tid] : 0x7fffffff;
            for (int size = 2; size <= 64; size <<= 1)
                for (int stride = size >> 1; stride > 0; stride >>= 1) {
                    const unsigned uo = __shfl_xor(u, stride);
                    const int io = __shfl_xor(ix, stride);
                    const bool lower = (tid & stride) == 0;            // this lane keeps the pair's first element ...
                    const bool up = (tid & size) == 0;                 // ... of a "best first" run
                    const bool mine_first = before(u, ix, uo, io);
                    const bool keep = (lower == up) ? mine_first : !mine_first;
                    if (!keep) {
                        u = uo;
                        ix = io;
                    }
                }
            if (tid < k) emit(tid, ix, u);
        }
        return;
    }
    for (int size = 2; size <= P; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int x = tid; x < P / 2; x += TK_THREADS) {
                const int a = 2 * x - (x & (stride - 1)), b = a + stride;
                const bool up = ((a & size) == 0);  // this pair's run is sorted "best first"
                const unsigned ua = cand_u[a], ub = cand_u[b];
                const int ia = cand_i[a], ib = cand_i[b];
                if (before(ub, ib, ua, ia) == up) {
                    cand_u[a] = ub; cand_i[a] = ib;
                    cand_u[b] = ua; cand_i[b] = ia;
                }
            }
            __syncthreads();
        }
    }
    for (int x = tid; x < k; x += TK_THREADS) emit(x, cand_i[x], cand_u[x]);
}

}  // namespace

int launch_topk(const float* scores, int64_t* idx, float* vals, int64_t B, int64_t N, int64_t k, hipStream_t st) {
    if (k < 1 || k > N || k > TK_MAXK || N >= (1ll << 31) || B >= (1ll << 31)) return NW_ERR_UNSUPPORTED;
    if (B == 0) return NW_OK;
    if (N <= 16 * TK_THREADS)
        hipLaunchKernelGGL((nw_topk_kernel<16>), dim3((unsigned)B), dim3(TK_THREADS), 0, st, scores, idx, vals, (int)N, (int)k, (const int*)nullptr);
    else if (N <= 32 * TK_THREADS)
        hipLaunchKernelGGL((nw_topk_kernel<32>), dim3((unsigned)B), dim3(TK_THREADS), 0, st, scores, idx, vals, (int)N, (int)k, (const int*)nullptr);
    else if (N <= 64 * TK_THREADS)
        hipLaunchKernelGGL((nw_topk_kernel<64>), dim3((unsigned)B), dim3(TK_THREADS), 0, st, scores, idx, vals, (int)N, (int)k, (const int*)nullptr);
    else
        hipLaunchKernelGGL((nw_topk_kernel<0>), dim3((unsigned)B), dim3(TK_THREADS), 0, st, scores, idx, vals, (int)N, (int)k, (const int*)nullptr);
    NW_CHECK_LAUNCH();
    return NW_OK;
}

int launch_topk_candidates(const unsigned* keys, const int* rows, int64_t* idx, float* vals, int64_t B, int64_t M, int64_t k,
                           hipStream_t st, bool pad_empty) {
    if (k < 1 || k > M || k > TK_MAXK || M >= (1ll << 31) || B >= (1ll << 31)) return NW_ERR_UNSUPPORTED;
    if (B == 0) return NW_OK;
    const float* kf = reinterpret_cast<const float*>(keys);
#define NW_TOPK_MAPPED(R_)                                                                                                  \
    if (pad_empty)                                                                                                          \
        hipLaunchKernelGGL((nw_topk_kernel<R_, true, true>), dim3((unsigned)B), dim3(TK_THREADS), 0, st, kf, idx, vals, (int)M, \
                           (int)k, rows);                                                                                   \
    else                                                                                                                    \
        hipLaunchKernelGGL((nw_topk_kernel<R_, true>), dim3((unsigned)B), dim3(TK_THREADS), 0, st, kf, idx, vals, (int)M, (int)k, rows)
    if (M <= 16 * TK_THREADS) { NW_TOPK_MAPPED(16); }
    else if (M <= 32 * TK_THREADS) { NW_TOPK_MAPPED(32); }
    else if (M <= 64 * TK_THREADS) { NW_TOPK_MAPPED(64); }
    else { NW_TOPK_MAPPED(0); }
#undef NW_TOPK_MAPPED
    NW_CHECK_LAUNCH();
    return NW_OK;
}

}  // namespace nw
