// knn_merge.hip -- the k nearest supports of every query over a SHARDED bank, and the NW head over them (gfx950 / MI355X only).
//
// Every shard has searched its own rows (nw_knn_f32 / nw_topk_f32) and left, per query, a list of kc candidates sorted best
// first -- (score, global bank row, global class id).  This kernel is the cross-shard step: per query a G-way merge of the G
// sorted lists to the k best overall, in nw_topk_kernel's order (score descending on ordered_bits, equal scores by ascending
// global row), then the per-query k-NN head of NWNet(knn_per_query=True) over the winners:
//   out[b][c] = log( sum_{j < k, label_j == c} softmax_j(val[b][0..k)) + 1e-12 )          (nw.py:285-289 on k supports)
//
// One wave per query (one 64-thread workgroup).  The wave first stages the query's G kc candidates in LDS as 64-bit keys
//   (ordered_bits(score) << 32) | (0x7fffffff - row)            0: "no element" (ordered_bits is never 0, topk.hip)
// so that "better" is plain unsigned "larger".  Lane g then holds the head of shard g's list in a register; each of the k
// rounds is a wave-wide maximum of the heads (a butterfly of shuffles: every lane ends with the same winner), and the one
// lane whose head won steps to its next element -- the only LDS read of the round.  Lane j keeps the winner of round j.
// Then lanes 0..k-1 fetch (score, label) of their winners, the wave takes the maximum, exp, the sum, and the classes are
// summed in neighbour order j = 0..k-1 by the lane that owns the class: no atomics, bit-reproducible.
#include "nw_internal.h"

namespace nw {
namespace {

constexpr int KM_MAXG = 64;   // shards: one lane each
constexpr int KM_MAXK = 32;   // neighbours (and candidates per shard): nw_knn_f32's limit

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned hi = __shfl_xor((unsigned)(v >> 32), o), lo = __shfl_xor((unsigned)v, o);
        const unsigned long long w = ((unsigned long long)hi << 32) | lo;
        v = w > v ? w : v;
    }
    return v;
}

__global__ __launch_bounds__(64) void nw_knn_merge_kernel(const float* __restrict__ vals, const int* __restrict__ rows,
                                                          const int* __restrict__ labels, int G, int kc, int64_t stride_g,
                                                          int k, int64_t C, int64_t* __restrict__ idx_out,
                                                          float* __restrict__ val_out, int64_t* __restrict__ label_out,
                                                          float* __restrict__ out) {
    extern __shared__ unsigned long long cand[];   // G kc keys (at most 16 KB; sized by the launch, for the occupancy of small merges)
    __shared__ float sh_e[KM_MAXK];
    __shared__ int sh_y[KM_MAXK];
    const int lane = threadIdx.x;
    const int64_t b = blockIdx.x;
    const int64_t qoff = b * kc;   // the query's list inside a shard's (B, kc) block

    // ---- stage the G lists: coalesced, independent loads (slot i = g kc + p)
    for (int i = lane; i < G * kc; i += 64) {
        const int g = i / kc, p = i - g * kc;
        const int64_t a = (int64_t)g * stride_g + qoff + p;
        const int r = rows[a];
        const unsigned key = ordered_bits(vals[a]);
        cand[i] = r >= 0 ? ((unsigned long long)key << 32) | (unsigned)(0x7fffffff - r) : 0ull;
    }
    __syncthreads();

    // ---- G-way merge: lane g offers the head of list g (a no-element slot ends its list)
    int pos = 0;
    unsigned long long head = lane < G ? cand[lane * kc] : 0ull;
    int my_row = -1, my_slot = 0;   // lane j: the winner of round j
    for (int j = 0; j < k; ++j) {
        const unsigned long long best = wave_max_u64(head);
        if (best == 0ull) break;   // (wave-uniform) every list is exhausted: the remaining slots stay "no element"
        const bool win = head == best;   // rows are unique: one lane
        const int slot = __shfl(lane * kc + pos, __builtin_ctzll(__ballot(win)));
        if (lane == j) {
            my_row = 0x7fffffff - (int)(unsigned)best;
            my_slot = slot;
        }
        if (win) {
            ++pos;
            head = pos < kc ? cand[lane * kc + pos] : 0ull;
        }
    }

    // ---- lanes 0..k-1: the score and label of their winner, as they stand in the lists
    const bool valid = lane < k && my_row >= 0;
    float v = -INFINITY;
    int y = -1;
    if (valid) {
        const int g = my_slot / kc;
        const int64_t a = (int64_t)g * stride_g + qoff + (my_slot - g * kc);
        v = vals[a];
        y = labels[a];
    }
    if (lane < k) {
        idx_out[b * k + lane] = valid ? (int64_t)my_row : (int64_t)-1;
        if (val_out) val_out[b * k + lane] = v;
        if (label_out) label_out[b * k + lane] = (int64_t)y;
    }
    if (!out || C <= 0) return;

    // ---- the head over the valid winners (nw_aggregate_kernel's arithmetic on a row of k scores)
    const float m = wave_max(v);
    const float e = valid ? expf(v - m) : 0.f;
    const float den = wave_sum(e);
    const float inv_den = den == 0.f ? 0.f : 1.f / den;   // no neighbour at all: log(0 + 1e-12), like N == 0
    if (lane < KM_MAXK) {
        sh_e[lane] = e;
        sh_y[lane] = valid ? y : -1;
    }
    __syncthreads();
    for (int64_t c = lane; c < C; c += 64) {
        float a = 0.f;
        for (int j = 0; j < k; ++j) a += ((int64_t)sh_y[j] == c) ? sh_e[j] : 0.f;   // (the same LDS word in every lane: a broadcast)
        out[b * C + c] = logf(a * inv_den + NW_LOG_EPS);
    }
}

}  // namespace

int launch_knn_merge(const float* vals, const int* rows, const int* labels, int64_t G, int64_t B, int64_t kc, int64_t stride_g,
                     int64_t k, int64_t C, int64_t* idx, float* val_out, int64_t* label_out, float* out, hipStream_t st) {
    if (k < 1 || k > KM_MAXK || kc < k || kc > KM_MAXK || G < 1 || G > KM_MAXG || B >= (1ll << 31)) return NW_ERR_UNSUPPORTED;
    if (B == 0) return NW_OK;
    const size_t lds = (size_t)(G * kc) * sizeof(unsigned long long);
    hipLaunchKernelGGL(nw_knn_merge_kernel, dim3((unsigned)B), dim3(64), lds, st, vals, rows, labels, (int)G, (int)kc, stride_g,
                       (int)k, C, idx, val_out, label_out, out);
    NW_CHECK_LAUNCH();
    return NW_OK;
}

}  // namespace nw
