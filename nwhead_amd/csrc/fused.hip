// fused.hip -- the fused NW-head forward for a shared (N,d) support (gfx950 / MI355X only).
//
// Replaces, in ONE pass over the support rows and without materialising the (B,N) score matrix,
// the reference sequence  one_hot -> kernel scores -> softmax -> bmm -> log  (nwhead/nw.py:276-289,
// scores from nwhead/kernel.py:13-44):
//
//   nw_fused_kernel   per workgroup tile (64 queries x 16*RS supports): fp32-MFMA dot products
//                     (tile_core.h), score epilogue, tile-local softmax statistics
//                     m = max_j s, den = sum_j e^(s-m), and the e^(s-m) sums of every RUN of equal
//                     consecutive labels inside the tile (a class-sorted bank has 1-2 runs per tile;
//                     an unsorted one degrades gracefully to one run per support).
//   nw_merge_runs_kernel  per query: rescale every tile to the global max, add run sums into the
//                     per-class accumulator, write log(num/den + 1e-12) (or the (m, den, num)
//                     partials of a shard).
#include <mutex>
#include <utility>
#include <vector>
#include "fused_impl.h"

namespace nw {

// instantiated in fused_k0.hip .. fused_k4.hip
#define NW_EXTERN_FUSED_KIND(K) extern template int launch_fused_kind<K>(const FusedArgs&, const FusedPlan&);
NW_FOR_EACH_KIND(NW_EXTERN_FUSED_KIND)
#undef NW_EXTERN_FUSED_KIND

// ---- diagnostics: device time of the tile kernel alone (nw_debug_tile_timing*, include/nwhead_hip.h)
namespace {
struct TileTimer {
    bool on = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev;  // pairs recorded since the last read
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pool;
    std::mutex mu;
} g_tt;
}  // namespace

int tile_timer_start(hipStream_t st) {
    if (!g_tt.on) return -1;
    std::lock_guard<std::mutex> lk(g_tt.mu);
    std::pair<hipEvent_t, hipEvent_t> p;
    if (!g_tt.pool.empty()) {
        p = g_tt.pool.back();
        g_tt.pool.pop_back();
    } else if (hipEventCreate(&p.first) != hipSuccess || hipEventCreate(&p.second) != hipSuccess) {
        return -1;
    }
    (void)hipEventRecord(p.first, st);
    g_tt.ev.push_back(p);
    return (int)g_tt.ev.size() - 1;
}
void tile_timer_stop(int slot, hipStream_t st) {
    if (slot < 0) return;
    std::lock_guard<std::mutex> lk(g_tt.mu);
    if (slot < (int)g_tt.ev.size()) (void)hipEventRecord(g_tt.ev[slot].second, st);
}
int tile_timer_enable(bool on) {
    std::lock_guard<std::mutex> lk(g_tt.mu);
    g_tt.on = on;
    return NW_OK;
}
int tile_timer_read(double* total_us, int64_t* launches) {
    std::lock_guard<std::mutex> lk(g_tt.mu);
    double tot = 0;
    for (auto& p : g_tt.ev) {
        float ms = 0.f;
        if (hipEventSynchronize(p.second) != hipSuccess || hipEventElapsedTime(&ms, p.first, p.second) != hipSuccess)
            return NW_ERR_LAUNCH;
        tot += (double)ms * 1e3;
        g_tt.pool.push_back(p);
    }
    if (total_us) *total_us = tot;
    if (launches) *launches = (int64_t)g_tt.ev.size();
    g_tt.ev.clear();
    return NW_OK;
}

namespace {
// The device property and the on/off knob the launch decision reads (plan_fused).
int device_cu_count() {
    static int n = [] {
        int dev = 0, v = 0;
        if (hipGetDevice(&dev) != hipSuccess) return 256;
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) return 256;
        return v;
    }();
    return n;
}
bool env_flag(int k) { return knob(k) == 1; }
}  // namespace

inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }

size_t fused_layout(int64_t B, int64_t n_stiles, int BS, char* base, FusedWs* ws, int64_t C) {
    size_t off = 0;
    auto take = [&](size_t bytes) {
        char* p = base ? base + off : nullptr;
        off += al256(bytes);
        return p;
    };
    FusedWs w;
    // (den follows m at the distance the OUT_WIN tile kernel assumes: both sides read fused_den_after_m)
    w.m = reinterpret_cast<float*>(take(fused_den_after_m(n_stiles, B) * sizeof(float)));
    w.den = reinterpret_cast<float*>(take((size_t)n_stiles * B * 4));
    w.nrun = reinterpret_cast<int*>(take((size_t)n_stiles * 4));
    w.lab = reinterpret_cast<int*>(take((size_t)n_stiles * BS * 4));
    w.num = reinterpret_cast<float*>(take((size_t)n_stiles * BS * B * 4));
    w.runid = reinterpret_cast<int*>(take(((size_t)n_stiles * BS + 64) * 4));
    w.bnd = reinterpret_cast<int*>(take((size_t)n_stiles * 2 * 4));
    w.ctab = reinterpret_cast<int*>(take((size_t)C * (3 + 4) * 4));   // class tables of the run merge when they do not fit in LDS
    if (ws) *ws = w;
    return off;
}

namespace {

// The run merge.  One workgroup per MQ consecutive queries; ws_m is in base-2 units (u = score * log2 e,
// see nw_fused_kernel).  Three phases, two global round trips, NO float atomics -- every sum has a fixed
// order, so the output is bit-reproducible from launch to launch:
//   0  (tables, shared by the workgroup's queries) per class c: the (tile, run) entries that carry it, in
//      bank order.  A class-sorted bank gives a class 1-3 entries; up to MENT are kept in LDS (integer LDS
//      atomics hand out the slots, the slots are then sorted: deterministic), a class with more entries is
//      found again by scanning the run labels of tiles [tlo[c], thi[c]].
//   1  M = max over tiles, den = sum_t den_t 2^(m_t - M): threads = MQ queries x ML tile lanes, each lane
//      sums its tiles in order, the lanes are added in order.
//   2  thread per (class, query): its entries' run sums, rescaled, added in bank order; every address is
//      known from the LDS tables, so the loads of one thread fly together.
// The reads of phases 0 and 1 do not depend on each other: one round trip; phase 2 is the second.
// (History: one LDS float atomicAdd per (tile, run) was 6.2 us at T and not reproducible; merging inside
//  the tile kernel -- the last workgroup of a query tile does it -- was tried and dropped: one CU's ~450
//  dependent-latency loads take 25 us, and agent-scope release/acquire fences cost ~40 us per launch on
//  the 8-XCD part.  A query-blocked workspace with packed run rows was measured too: no change.)
constexpr int MTHREADS = 512, MENT = 4, MTPT = 16;
// TMODE: where the per-class tables (count, first / last tile, up to MENT entries) live: 1 = LDS, built by every
// workgroup (they fit up to a few thousand classes); 2 = global memory, built once per launch by
// nw_class_tables_kernel (more classes than LDS holds: MQ = 1, results written directly).  (0 was "no tables, every class
// scans every tile": 4.9 ms per call at T, and fused_layout always carves the workspace that mode 2 needs.)
template <bool PARTIAL, int MQ, int TMODE>
__global__ __launch_bounds__(MTHREADS) void nw_merge_runs_kernel(
    const float* __restrict__ ws_m, const float* __restrict__ ws_den, const int* __restrict__ ws_nrun,
    const int* __restrict__ ws_lab, const float* __restrict__ ws_num, float* __restrict__ out,
    float* __restrict__ lse, float* __restrict__ m_out, float* __restrict__ den_out,
    float* __restrict__ num_out, int B, int C, int n_stiles, int BS, const int* __restrict__ ctab) {
    static_assert(TMODE == 1 || TMODE == 2, "the per-class tables live in LDS (1) or in the workspace (2)");
    constexpr bool LTAB = TMODE == 1;   // tables built here, in LDS
    constexpr int ML = MTHREADS / MQ;  // tile lanes per query
    constexpr int MNS = MQ + 1;        // row stride of res[class][query] in LDS: odd, the output phase reads columns
    constexpr int NW = MTHREADS / 64;  // waves
    constexpr float LN2 = 0.693147180559945309417f;
    static_assert(MQ <= 32 && (MQ & (MQ - 1)) == 0, "a wave holds whole groups of MQ queries");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* red = reinterpret_cast<float*>(smem);  // [NW][MQ] x 2
    float* Ms = red + 2 * NW * MQ;                // [MQ]
    float* inv_s = Ms + MQ;                       // [MQ]
    int* lds_tab = reinterpret_cast<int*>(inv_s + MQ);
    int* cnt = TMODE == 2 ? const_cast<int*>(ctab) : lds_tab;  // [C]   entries of class c
    int* tlo = cnt + C;                             // [C]   first tile carrying c
    int* thi = tlo + C;                             // [C]   last tile carrying c
    int* ent = thi + C;                             // [C][MENT]  tile * BS + run, ascending
    float* res = reinterpret_cast<float*>(lds_tab + (size_t)C * (3 + MENT));  // [C][MNS]   (LDS tables, MQ > 1)
    const int tid = threadIdx.x, bq = tid & (MQ - 1), sl = tid / MQ, wave = tid >> 6;
    const int b0 = blockIdx.x * MQ;
    const int b = min(b0 + bq, B - 1);  // rows past the batch repeat the last query and are never written

    // ---- round trip 1: this thread's tiles (kept in registers when there are at most MTPT of them) and the
    // run tables.  The first three run labels of a tile are read before its run count is known (rows past nrun
    // are allocated, never written: what comes back is selected away).
    const bool in_regs = n_stiles <= ML * MTPT;
    float mr[MTPT], dr[MTPT];
    float M = -INFINITY;
    if (in_regs) {
#pragma unroll
        for (int u = 0; u < MTPT; ++u) {
            const int t = sl + u * ML;
            const bool ok = t < n_stiles;
            mr[u] = ok ? ws_m[(size_t)t * B + b] : -INFINITY;
            dr[u] = ok ? ws_den[(size_t)t * B + b] : 0.f;
        }
    }
    int tnr = 0, tl3[3] = {-1, -1, -1};
    const bool one_pass_tables = LTAB && n_stiles <= MTHREADS;
    if (one_pass_tables && tid < n_stiles) {
        tnr = ws_nrun[tid];
        const int* lt = ws_lab + (size_t)tid * BS;
        tl3[0] = lt[0];
        tl3[1] = lt[1];
        tl3[2] = lt[2];
    }
    if (LTAB) {
        for (int c = tid; c < C; c += MTHREADS) {
            cnt[c] = 0;
            tlo[c] = 0x7fffffff;
            thi[c] = -1;
        }
    }
    if (in_regs) {
#pragma unroll
        for (int u = 0; u < MTPT; ++u) M = fmaxf(M, mr[u]);
    } else {
        for (int t = sl; t < n_stiles; t += ML) M = fmaxf(M, ws_m[(size_t)t * B + b]);
    }
#pragma unroll
    for (int o = 32; o >= MQ; o >>= 1) M = fmaxf(M, __shfl_xor(M, o));  // lanes l, l ^ MQ, ... hold the same query
    if ((tid & 63) < MQ) red[wave * MQ + bq] = M;
    __syncthreads();  // also publishes the reset tables
    // ---- phase 0: class tables
    if (LTAB) {
        auto add_tile = [&](int t, int nr, const int (&l3)[3]) {
            const int* lt = ws_lab + (size_t)t * BS;
            for (int r = 0; r < nr; ++r) {
                const int y = r < 3 ? l3[r] : lt[r];
                if (y < 0) continue;  // padding rows / labels outside [0, C)
                atomicMin(&tlo[y], t);
                atomicMax(&thi[y], t);
                const int slot = atomicAdd(&cnt[y], 1);
                if (slot < MENT) ent[y * MENT + slot] = t * BS + r;
            }
        };
        if (one_pass_tables) {
            if (tid < n_stiles) add_tile(tid, tnr, tl3);
        } else {
            for (int t = tid; t < n_stiles; t += MTHREADS) {
                const int* lt = ws_lab + (size_t)t * BS;
                const int l3[3] = {lt[0], lt[1], lt[2]};
                add_tile(t, ws_nrun[t], l3);
            }
        }
    }
    M = red[bq];
#pragma unroll
    for (int k = 1; k < NW; ++k) M = fmaxf(M, red[k * MQ + bq]);
    // A query whose row window admits no row at all (OUT_WIN) has m = -inf and den = 0 in every tile.  Its rescaling runs
    // against 0 (2^(-inf - 0) = 0 where -inf - -inf would be NaN) and its 1 / den below is 0: every class comes out as
    // log(NW_LOG_EPS) and lse as -inf.  Every other call has a finite M and den >= 1, and both selects leave them as they are.
    const bool no_rows = M == -INFINITY;
    if (no_rows) M = 0.f;
    // ---- den: every thread adds its tiles in order, the tile lanes of a wave are added in a fixed tree, the
    // waves in order
    float den = 0.f;
    if (in_regs) {
#pragma unroll
        for (int u = 0; u < MTPT; ++u) den += dr[u] * __builtin_amdgcn_exp2f(mr[u] - M);  // absent tiles: 0 * 2^-inf = 0
    } else {
        for (int t = sl; t < n_stiles; t += ML)
            den += ws_den[(size_t)t * B + b] * __builtin_amdgcn_exp2f(ws_m[(size_t)t * B + b] - M);
    }
#pragma unroll
    for (int o = 32; o >= MQ; o >>= 1) den += __shfl_xor(den, o);
    if ((tid & 63) < MQ) red[NW * MQ + wave * MQ + bq] = den;
    if (sl == 0) Ms[bq] = M;
    __syncthreads();  // partial dens and the class tables are complete
    if (LTAB) {  // slots were handed out in arrival order: put each class's entries in bank order
        for (int c = tid; c < C; c += MTHREADS) {
            const int n = cnt[c];
            if (n > 1 && n <= MENT) {
                int e[MENT];
#pragma unroll
                for (int k = 0; k < MENT; ++k) e[k] = k < n ? ent[c * MENT + k] : 0x7fffffff;
#pragma unroll
                for (int i = 1; i < MENT; ++i)
#pragma unroll
                    for (int j = MENT - 1; j >= i; --j)
                        if (e[j] < e[j - 1]) { const int x = e[j]; e[j] = e[j - 1]; e[j - 1] = x; }
#pragma unroll
                for (int k = 0; k < MENT; ++k)
                    if (k < n) ent[c * MENT + k] = e[k];
            }
        }
    }
    den = red[NW * MQ + bq];
#pragma unroll
    for (int k = 1; k < NW; ++k) den += red[NW * MQ + k * MQ + bq];
    if (sl == 0) inv_s[bq] = no_rows ? 0.f : 1.f / den;
    const int nq = min(MQ, B - b0);
    if (sl == 0 && bq < nq) {
        if (PARTIAL) {
            m_out[b] = M * LN2;  // back to natural units
            den_out[b] = den;
        } else if (lse) {
            lse[b] = M * LN2 + logf(den);
        }
    }
    __syncthreads();  // sorted entries, inv_s
    // ---- round trip 2: class sums.  Few classes (C * MQ well under the workgroup's 512 threads) mean many tiles per
    // class: P lanes then share one (class, query) item -- lane `sub` takes the tiles t0 + sub, t0 + sub + P, ... and the
    // P partial sums are added in a fixed shuffle tree (a single class over 63 tiles: 36 -> 9 us of merge at T).
    int P = 1;
    while (P < 64 && 2 * P * C * MQ <= MTHREADS) P <<= 1;
    for (int xx = tid; xx < C * MQ * P; xx += MTHREADS) {
        const int x = xx / P, sub = xx - x * P;
        const int c = x / MQ, q = x - c * MQ;
        const int bb = min(b0 + q, B - 1);
        const float Mq = Ms[q];
        float acc = 0.f;
        const int n = cnt[c];
        if (n <= MENT) {
            int e[MENT];
            float v[MENT], mt[MENT];
#pragma unroll
            for (int k = 0; k < MENT; ++k) e[k] = ent[c * MENT + (k < n ? k : 0)];
#pragma unroll
            for (int k = 0; k < MENT; ++k) {
                if (k < n) {
                    v[k] = ws_num[(size_t)e[k] * B + bb];
                    mt[k] = ws_m[(size_t)(e[k] / BS) * B + bb];
                }
            }
#pragma unroll
            for (int k = 0; k < MENT; ++k)
                if (k < n) acc += v[k] * __builtin_amdgcn_exp2f(mt[k] - Mq);
        } else {
            const int t0 = tlo[c], t1 = thi[c];
            for (int t = t0 + sub; t <= t1; t += P) {
                const int nr = ws_nrun[t];
                const float f = __builtin_amdgcn_exp2f(ws_m[(size_t)t * B + bb] - Mq);
                const int* lt = ws_lab + (size_t)t * BS;
                for (int r = 0; r < nr; ++r)
                    if (lt[r] == c) acc += ws_num[((size_t)t * BS + r) * B + bb] * f;
            }
        }
        if (P > 1) {   // (every lane of the item's group is here: groups are whole, the loop bounds are theirs alike)
            if (n <= MENT && sub != 0) acc = 0.f;
            for (int o = P >> 1; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
            if (sub != 0) continue;
        }
        if (LTAB && MQ > 1) {
            res[c * MNS + q] = acc;
        } else if (q < nq) {  // one query per workgroup (consecutive classes: coalesced), or no room for the staging table
            if (PARTIAL) num_out[(size_t)bb * C + c] = acc;
            else out[(size_t)bb * C + c] = logf(acc * inv_s[q] + NW_LOG_EPS);
        }
    }
    if (!LTAB || MQ == 1) return;
    __syncthreads();
    for (int x = tid; x < nq * C; x += MTHREADS) {
        const int qq = x / C, c = x - qq * C;
        if (PARTIAL) num_out[(size_t)(b0 + qq) * C + c] = res[c * MNS + qq];
        else out[(size_t)(b0 + qq) * C + c] = logf(res[c * MNS + qq] * inv_s[qq] + NW_LOG_EPS);
    }
}

// The run merge's per-class tables in GLOBAL memory (ctab = cnt[C] | tlo[C] | thi[C] | ent[C][MENT]), for class counts
// whose tables do not fit in LDS: built once per launch by ONE workgroup (the tables depend on the labels and the
// tiling only, not on the queries), integer atomics hand out the slots, then every class's entries are put in bank
// order -- the same construction nw_merge_runs_kernel does per workgroup in LDS.
__global__ __launch_bounds__(1024) void nw_class_tables_kernel(const int* __restrict__ ws_nrun, const int* __restrict__ ws_lab,
                                                                int n_stiles, int BS, int C, int* __restrict__ ctab) {
    int* cnt = ctab;
    int* tlo = cnt + C;
    int* thi = tlo + C;
    int* ent = thi + C;
    const int tid = threadIdx.x;
    for (int c = tid; c < C; c += 1024) {
        cnt[c] = 0;
        tlo[c] = 0x7fffffff;
        thi[c] = -1;
    }
    __threadfence();
    __syncthreads();
    for (int t = tid; t < n_stiles; t += 1024) {
        const int nr = ws_nrun[t];
        const int* lt = ws_lab + (size_t)t * BS;
        for (int r = 0; r < nr; ++r) {
            const int y = lt[r];
            if (y < 0) continue;
            atomicMin(&tlo[y], t);
            atomicMax(&thi[y], t);
            const int slot = atomicAdd(&cnt[y], 1);
            if (slot < MENT) ent[y * MENT + slot] = t * BS + r;
        }
    }
    __threadfence();
    __syncthreads();
    for (int c = tid; c < C; c += 1024) {
        const int n = cnt[c];
        if (n > 1 && n <= MENT) {
            int e[MENT];
#pragma unroll
            for (int k = 0; k < MENT; ++k) e[k] = k < n ? ent[c * MENT + k] : 0x7fffffff;
#pragma unroll
            for (int i = 1; i < MENT; ++i)
#pragma unroll
                for (int j = MENT - 1; j >= i; --j)
                    if (e[j] < e[j - 1]) { const int x = e[j]; e[j] = e[j - 1]; e[j - 1] = x; }
#pragma unroll
            for (int k = 0; k < MENT; ++k)
                if (k < n) ent[c * MENT + k] = e[k];
        }
    }
}

// Runs of equal consecutive labels inside every support tile of BS rows, one wave per tile:
// runid[st*BS + t] = run of tile row t, lab[st*BS + run] = its class (-1: padding rows / labels outside
// [0, C)), nrun[st].  The persistent kernel reads these instead of scanning the labels once per
// (query tile, support tile) pair.
__global__ __launch_bounds__(64) void nw_run_tables_kernel(const int64_t* __restrict__ sy, int N, int C, int BS,
                                                           int* __restrict__ runid, int* __restrict__ nrun,
                                                           int* __restrict__ lab_out, int* __restrict__ bnd) {
    const int st = blockIdx.x, lane = threadIdx.x, s0 = st * BS;
    if (lane < 2) bnd[2 * st + lane] = BS;  // overwritten below when runs 1 / 2 exist (same lane order: see the barrier)
    __syncthreads();
    int lab[3], flag[3];
#pragma unroll
    for (int u = 0; u < 3; ++u) {
        const int t = 3 * lane + u, j = s0 + t;
        int64_t y = -1;
        if (t < BS && j < N) y = sy[j];
        lab[u] = ((uint64_t)y < (uint64_t)C) ? (int)y : -1;
    }
    const int prev_last = __shfl_up(lab[2], 1);
    flag[0] = (lane == 0) || (lab[0] != prev_last);
    flag[1] = lab[1] != lab[0];
    flag[2] = lab[2] != lab[1];
    int incl = flag[0] + flag[1] + flag[2];
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(incl, o);
        if (lane >= o) incl += v;
    }
    int id = incl - (flag[0] + flag[1] + flag[2]) - 1;
#pragma unroll
    for (int u = 0; u < 3; ++u) {
        const int t = 3 * lane + u;
        id += flag[u];
        if (t < BS) {
            runid[(size_t)s0 + t] = id;
            if (flag[u]) lab_out[(size_t)s0 + id] = lab[u];
            if (flag[u] && (id == 1 || id == 2)) bnd[2 * st + id - 1] = t;
            if (t == BS - 1) nrun[st] = id + 1;
        }
    }
}

int env_rs() {
    const int v = knob(KNOB_TILE_RS);
    return v == KNOB_UNSET ? 0 : v;
}

}  // namespace

int launch_run_tables(const FusedWs& ws, const int64_t* sy, int N, int C, int n_stiles, int BS, hipStream_t st) {
    if (BS > 192) return NW_ERR_UNSUPPORTED;  // three rows per lane
    hipLaunchKernelGGL(nw_run_tables_kernel, dim3(n_stiles), dim3(64), 0, st, sy, N, C, BS, ws.runid, ws.nrun, ws.lab, ws.bnd);
    NW_CHECK_LAUNCH();
    return NW_OK;
}

// A resident bank's run tables, built once (nw_bank_tables_build) instead of once per forward.  They depend on the
// labels, N, C and the tile height only; the persistent kernel's tile is 128 supports.  The caller passes them with the
// call (nw_fwd_opts.tables): they must be the tables of the very label array, N and C of that call.
constexpr int BANK_BS = 128;

size_t bank_tables_layout(int64_t n_stiles, char* base, FusedWs* ws) {
    size_t off = 0;
    auto take = [&](size_t bytes) {
        char* p = base ? base + off : nullptr;
        off += al256(bytes);
        return p;
    };
    int* nrun = reinterpret_cast<int*>(take((size_t)n_stiles * 4));
    int* lab = reinterpret_cast<int*>(take((size_t)n_stiles * BANK_BS * 4));
    int* runid = reinterpret_cast<int*>(take(((size_t)n_stiles * BANK_BS + 64) * 4));
    int* bnd = reinterpret_cast<int*>(take((size_t)n_stiles * 2 * 4));
    if (ws) {
        ws->nrun = nrun;
        ws->lab = lab;
        ws->runid = runid;
        ws->bnd = bnd;
    }
    return off;
}

bool bank_tables_take(const int64_t* sy, int N, int C, int n_stiles, int BS, FusedWs* ws) {
    (void)C;   // (the tables do not depend on the class count: labels >= C are the caller's check, as in nw_bank_tables_build)
    const FwdOpts& o = fwd_opts();
    if (!o.tables || BS != BANK_BS) return false;
    if (o.tables_sy != sy || o.tables_N != (int64_t)N) return false;   // tables of another label array: build our own
    if (o.tables_bytes < bank_tables_layout(n_stiles, nullptr, nullptr)) return false;
    bank_tables_layout(n_stiles, const_cast<char*>(o.tables), ws);
    return true;
}

int launch_merge_runs(const FusedWs& ws, float* out, float* lse, float* m, float* den, float* num,
                      int B, int C, int n_stiles, int BS, hipStream_t st) {
    // LDS: reduction scratch + per-class tables (count, first / last tile, MENT entries) + res[class][query]
    auto lds_bytes = [&](int mq, bool tables) {
        return ((size_t)2 * (MTHREADS / 64) * mq + 2 * mq + (tables ? (size_t)C * (3 + MENT + mq + 1) : 0)) * sizeof(float);
    };
    const size_t cap = 150 * 1024;
    // 32 queries x 16 tile lanes per workgroup when a query has few tiles (a shard of the bank), else 16 x 32;
    // below 512 queries one workgroup per query (T: 256 workgroups, one per CU)
    int mq = 1;
    if (B >= 512) {
        mq = n_stiles >= 128 ? 16 : 32;
        if (lds_bytes(mq, true) > cap) mq = 16;
        if (lds_bytes(mq, true) > cap) mq = 1;
    }
    const bool tables = lds_bytes(mq, true) <= cap;
    const size_t lds = lds_bytes(mq, tables);
    const int grid = (B + mq - 1) / mq;
#define NW_MERGE(P_, Q_, T_)                                                                                       \
    hipLaunchKernelGGL((nw_merge_runs_kernel<P_, Q_, T_>), dim3(grid), dim3(MTHREADS), lds, st, ws.m, ws.den, ws.nrun, \
                       ws.lab, ws.num, out, lse, m, den, num, B, C, n_stiles, BS, ws.ctab)
    if (!tables) {
        // more classes than LDS holds tables for (C > ~4200): the tables go to the workspace, built once per launch
        // in ws.ctab, which fused_layout carves for every class count
        // (measured at C = 5000: 4.9 ms per call at T when every class scanned every tile, 35 ms at B = 4096, N = 50000)
        hipLaunchKernelGGL(nw_class_tables_kernel, dim3(1), dim3(1024), 0, st, ws.nrun, ws.lab, n_stiles, BS, C, ws.ctab);
        if (out) NW_MERGE(false, 1, 2); else NW_MERGE(true, 1, 2);
    } else if (mq == 1) {
        if (out) NW_MERGE(false, 1, 1); else NW_MERGE(true, 1, 1);
    } else if (mq == 16) {
        if (out) NW_MERGE(false, 16, 1); else NW_MERGE(true, 16, 1);
    } else {
        if (out) NW_MERGE(false, 32, 1); else NW_MERGE(true, 32, 1);
    }
#undef NW_MERGE
    NW_CHECK_LAUNCH();
    return NW_OK;
}

// Support-tile height (in 16-row blocks).  Model: workgroups run in rounds of 256 (one per CU at
// full MFMA rate; two co-resident ones share the pipe but fill each other's barrier bubbles, worth
// ~15 %), each costs RS blocks of MFMA work plus a fixed prologue/epilogue.
int pick_rs(int64_t B, int64_t N, int64_t d, bool f16) {
    const int forced = env_rs();
    if (forced == 2 || forced == 4 || forced == 5 || forced == 6 || forced == 8 || forced == 10 || forced == 12)
        return forced;
    const int64_t nq = (B + BQ - 1) / BQ;
    // LDS-DMA path (d % 32 == 0): 80-row tiles keep a workgroup under 80 KB of LDS and 128 VGPRs, so
    // two share a CU and hide each other's prologue, barriers and epilogue (measured 111.6 vs 105.2
    // TFLOP/s at B=2048 N=50000, 36.2 vs 37.0 us at T) -- worth it once they fill the 512 slots.
    // (the split-fp16 path is bound by the L2->LDS stream, not by the matrix pipe: the larger tile,
    //  which moves fewer bytes per flop, wins there: 470 vs 509 us at B=2048 N=50000)
    if (forced == 0 && !f16 && d % BK == 0 && nq * ((N + 79) / 80) >= 480) return 5;
    // split-fp16 with >= 4 tiles per CU: the persistent kernel (fused_f16p.h) at its no-spill height
    if (forced == 0 && f16 && d % BK == 0 && nq * ((N + 127) / 128) >= 4 * 256) return 8;
    const int cand[] = {2, 4, 6, 8, 10, 12};  // even: the four loader waves split a tile evenly
    const int ncand = f16 ? 5 : 6;           // split-fp16: 12 blocks of fragments do not fit 256 VGPRs
    double best = 1e30;
    int best_rs = 8;
    for (int ci = 0; ci < ncand; ++ci) {
        const int rs = cand[ci];
        const int64_t ns = (N + 16 * rs - 1) / (16 * rs);
        const int64_t nwg = nq * ns;
        const int64_t rounds = (nwg + 255) / 256;
        double cost = (double)rounds * (rs + 1.5);
        if (nwg >= 384) cost *= 0.85;
        if (cost < best - 1e-9) {
            best = cost;
            best_rs = rs;
        }
    }
    return best_rs;
}

bool half_form_shape_ok(int64_t d) {   // whole 64-k stages, at least three of them (fused_f16p12.h), tile-relative offsets
    return d % 64 == 0 && d >= 192 && d <= (1 << 20);
}

namespace {
struct TileLds {   // dynamic LDS of nw_fused_kernel at one tile height: register-staged / LDS-DMA loaders
    size_t reg, dma;
};
template <int RS>
constexpr TileLds tile_lds() {
    return {FUSED_HDR + TileCfg<RS>::STAGE_BYTES, FUSED_HDR + DmaCfg<RS>::STAGE_BYTES};
}
// nw_fused_f16p_kernel runs on tiles of 128 supports only (RS = 8): its variants 0, 1, 2.  Two workgroups of variant 1
// share a CU's LDS; one of variant 2 has it to itself.
constexpr size_t P64_LDS = PCfg<8, 1, false>::LDS_BYTES, P64X2_LDS = PCfg<8, 1, true>::LDS_BYTES,
                 P128_LDS = PCfg<8, 2, false>::LDS_BYTES;
static_assert(P128_LDS <= 160 * 1024 && P64X2_LDS <= 80 * 1024, "the LDS of one CU / of half a CU");
TileLds tile_lds_of(int rs) {
    return rs == 2 ? tile_lds<2>() : rs == 4 ? tile_lds<4>() : rs == 5 ? tile_lds<5>() : rs == 6 ? tile_lds<6>()
         : rs == 8 ? tile_lds<8>() : rs == 10 ? tile_lds<10>() : tile_lds<12>();
}
}  // namespace

FusedPlan plan_tiles(int64_t B, int64_t N, int64_t d, int form) {
    FusedPlan p = {};
    p.form = form;
    // nw_fwd_opts.operand_form = 1 runs on tiles of 128 supports at every size: the tile-count rule of pick_rs is a speed
    // heuristic, and that form has no other kernel
    p.rs = form == FORM_HALF ? BANK_BS / 16 : pick_rs(B, N, d, form == FORM_SPLIT);
    p.BS = 16 * p.rs;
    const int64_t n_stiles = (N + p.BS - 1) / p.BS, n_qtiles = (B + BQ - 1) / BQ;
    const int64_t grid = (n_stiles + 7) / 8 * 8 * n_qtiles;   // padded_grid
    // More tiles than a launch has workgroups: refused for every form, the persistent kernels included (new with the plan:
    // the launchers let the int grid overflow and launched; such a shape needs terabytes of workspace and cannot be served).
    if (grid > 0x7fffffff) p.status = NW_ERR_UNSUPPORTED;
    else p.n_stiles = (int)n_stiles, p.n_qtiles = (int)n_qtiles, p.grid = (int)grid;
    return p;
}

FusedPlan plan_fused(int64_t B, int64_t N, int64_t d, int64_t C, int form, int out, int k, bool norms, bool dot, int cus,
                     const FwdOpts& opts) {
    (void)C;   // (the class count sizes the merge; k sizes the candidate slots and bounds the half form's selection)
    if (B < 0 || N < 0 || d < 0 || B >= (1 << 30) || N >= (1 << 30) || d >= (1 << 30)) {   // (fused_eligible's limits)
        FusedPlan none = {};
        return none.status = NW_ERR_UNSUPPORTED, none;
    }
    FusedPlan p = plan_tiles(B, N, d, form);
    if (p.status != NW_OK) return p;
    auto refuse = [&p](int status) { p.status = status; return p; };
    if (cus <= 0) cus = device_cu_count();
    const TileLds lds = tile_lds_of(p.rs);
    const bool split = form == FORM_SPLIT;
    p.out = out;
    p.dma = (d % BK) == 0 && (uint64_t)(BQ + p.BS) * 2 * d * 4 < 0xffffffffull;  // per-lane offsets are tile-relative
    if (form == FORM_HALF) {
        // log-probabilities / partials, or candidates (the epilogue's selection holds 32 keys per query block); no
        // score-writing half kernel exists
        if ((out != OUT_NONE && out != OUT_CAND) || !half_form_shape_ok(d)) return refuse(NW_ERR_UNSUPPORTED);
        if (out == OUT_CAND && (k < 1 || k > 32)) return refuse(NW_ERR_UNSUPPORTED);
        p.persistent = true;
    } else {
        // RS = 5 exists for the LDS-DMA modes only (two workgroups per CU); the register-staged loaders need an even split
        // of the tile rows
        if (!p.dma && (p.rs & 1)) return refuse(NW_ERR_UNSUPPORTED);
        // many tiles per CU on split operands: the persistent kernel (fused_f16p.h).  RS = 8 is the tallest tile whose
        // build stays under 256 VGPRs, and the only height it is built for.
        p.persistent = split && out == OUT_NONE && p.rs == 8 && p.grid >= 4 * (int64_t)cus && d >= 3 * BK &&
                       !env_flag(KNOB_NO_PERSISTENT);
    }
    p.run_tables = p.persistent && out != OUT_CAND;   // runs of equal labels per support tile: once per launch, or the bank's
    if (p.run_tables && p.BS > 192) return refuse(NW_ERR_UNSUPPORTED);   // nw_run_tables_kernel: three rows per lane
    // split-fp16 operands: the caller has checked d % 32 == 0 and supplied the bank's norms
    if (split && (!p.dma || !norms)) return refuse(NW_ERR_INVALID_ARG);
    if (out == OUT_CAND && form == FORM_F32) return refuse(NW_ERR_INVALID_ARG);
    // (RS = 12 on split operands exists only under the tile_rs knob and spills there: no candidate form of it)
    if (out == OUT_CAND && split && p.rs == 12) return refuse(NW_ERR_UNSUPPORTED);
    // the windowed head: split rows on nw_fused_kernel only (p.persistent above asks for OUT_NONE: never the persistent
    // kernels, so never run tables either), at the tile heights of the candidate form
    // (OUT_WGT, the same with row weights: the same plan)
    if (out_is_win(out) && form == FORM_F32) return refuse(NW_ERR_INVALID_ARG);
    if (out_is_win(out) && p.rs == 12) return refuse(NW_ERR_UNSUPPORTED);
    if (p.persistent) {
        p.mode = MODE_F16;
        p.split_queries = true;
        int wgs = cus & ~7;  // the same number of workgroups on every XCD
        // nw_fwd_opts.persistent_wgs: fewer workgroups than CUs (a multiple of 8), to leave CUs to a concurrent RCCL kernel
        // of the sharded path (ShardedBank leaves one CU per XCD when there is more than one rank)
        const int wg_cap = opts.persistent_wgs & ~7;
        if (wg_cap >= 8 && wg_cap < wgs) wgs = wg_cap;
        // 0: 64-query tiles, one workgroup per CU; 1: two per CU; 2: 128-query tiles; 3: 256-query tiles on eight
        // multiplying waves (fused_f16p12.h, tiles of 128 supports only).  Measured at B = 2048, N = 50000, d = 512
        // (tools/bench_fused.hip, same device): 387 / 353 / 337 us for 0 / 1 / 2.  The tallest tile whose padding costs no
        // more than 15 % of the rows (else two 64-query workgroups per CU).
        int variant = form == FORM_HALF ? 3 : knob(KNOB_PVAR);   // NW_PVAR forces one of 0-3
        if (variant < 0 || variant > 3) {
            const double rows64 = 1.15 * ((B + 63) / 64 * 64);
            variant = ((B + 255) / 256 * 256 <= rows64) ? 3 : ((B + 127) / 128 * 128 <= rows64) ? 2 : 1;
        }
        p.variant = variant;
        p.workgroups = variant == 1 ? 2 * wgs : wgs;
        // query tiles kept L2-resident per XCD (NW_QG = 1..64, else 8); variant 3: the same bytes of queries as with
        // 128-query tiles
        const int qg = (knob(KNOB_QG) >= 1 && knob(KNOB_QG) <= 64) ? knob(KNOB_QG) : 8;
        p.qgroup = variant != 3 ? qg : qg >= 2 ? qg / 2 : 1;
        p.lds_bytes = variant == 3 ? (size_t)P12::LDS_BYTES : variant == 2 ? P128_LDS : variant == 1 ? P64X2_LDS : P64_LDS;
        return p;
    }
    if (split) {
        // Raw queries (MODE_F16Q) cost every workgroup a pass over its 64 query rows and the split in its loop
        // (~5.4 k cycles at T); the split launch costs ~4.4 us + a kernel boundary once.  Measured per forward
        // (N = 10000, d = 512; raw / split launch): B = 256 20.2 / 21.8 us, 512 40.6 / 40.1, 768 52.7 / 50.4, 1000
        // 62.4 / 62.3: raw up to 1.5 workgroups per CU.  NW_SPLIT_QUERIES=1 / 0 forces either.
        const int force_split = knob(KNOB_SPLIT_QUERIES) == KNOB_UNSET ? -1 : knob(KNOB_SPLIT_QUERIES);
        const bool raw_ok = force_split == 0 || (force_split < 0 && 2 * (int64_t)p.grid <= 3 * (int64_t)cus);
        p.split_queries = !raw_ok;
        p.mode = raw_ok ? MODE_F16Q : MODE_F16;
    } else {
        p.mode = !p.dma ? MODE_REG : (norms && !dot) ? MODE_DMA_SN : MODE_DMA;   // cached norms: nothing to add for DOT
    }
    p.lds_bytes = p.mode == MODE_REG ? lds.reg : lds.dma;
    return p;
}

static size_t fused_workspace_bytes(int64_t B, int64_t N, int64_t d, int64_t C) {
    size_t need = 0;
    for (int form : {FORM_F32, FORM_SPLIT, FORM_HALF}) {  // any operand form may be chosen at launch
        if (form == FORM_HALF && !half_form_shape_ok(d)) continue;
        const int BS = plan_tiles(B, N, d, form).BS;
        const size_t n = fused_layout(B, (N + BS - 1) / BS, BS, nullptr, nullptr, C);
        need = n > need ? n : need;
    }
    return need;
}

FwdLayout fwd_layout(int64_t B, int64_t N, int64_t d, int64_t C, void* base) {
    FwdLayout L = {};
    L.base = static_cast<char*>(base);
    if (B <= 0 || N <= 0) return L;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        const FwdLayout::Area a = {off, al256(bytes)};
        off += a.bytes;
        return a;
    };
    const size_t scores = (size_t)B * (size_t)N * sizeof(float), fused = fused_workspace_bytes(B, N, d, C);
    L.main = take(scores > fused ? scores : fused);
    L.q_rows = take((size_t)B * (size_t)d * sizeof(float));
    L.q_scale = take((size_t)B * sizeof(float));
    L.q_norm2 = take((size_t)B * sizeof(float));
    L.lse = take((size_t)B * sizeof(float));
    L.n_slices = aggregate_slices(B, N);
    L.slices = take(L.n_slices > 1 ? (size_t)L.n_slices * (size_t)B * (size_t)(2 + (C > 0 ? C : 0)) * sizeof(float) : 0);
    L.total = off;
    return L;
}

bool fused_eligible(const float* q, const float* s, int64_t B, int64_t N, int64_t d, int64_t C) {
    const bool aligned = ((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(s)) & 15) == 0;
    return N > 25 && d >= 4 && (d % 4) == 0 && aligned && B < (1 << 30) && N < (1 << 30) &&
           d < (1 << 30) && C < (1 << 30) && (8 + C) * 4 <= 160 * 1024;
}

int launch_fused(const FusedArgs& a, int form, int kind) {
    const int out = a.cand ? OUT_CAND : a.row_logw ? OUT_WGT : (a.win_lo && a.win_hi) ? OUT_WIN : a.scores ? OUT_SCORES : OUT_NONE;
    const FusedPlan p = plan_fused(a.B, a.N, a.d, a.C, form, out, a.cand ? a.cand->k : 0, a.s_norm2 != nullptr,
                                   kind == NW_SCORE_DOT, 0, fwd_opts());
#define NW_KIND_CASE(K) case K: return launch_fused_kind<K>(a, p);
    switch (kind) {
        NW_FOR_EACH_KIND(NW_KIND_CASE)
        default: return NW_ERR_UNSUPPORTED;
    }
#undef NW_KIND_CASE
}

// ---- nearest-neighbour search without the (B,N) score matrix (nw_knn_f32, nw_knn_window_f32, nw_knn_f16): the tile
// kernel's candidate output under the launch decision of the score-writing call of the same operand form, then the k best
// of every query's candidates (topk.hip).  FORM_SPLIT: nw_fused_kernel / the persistent kernel (fused_impl.h, OUT_CAND) on
// the tile height of pick_rs.  FORM_HALF: the candidate form of the persistent 256-query kernel (fused_f16p12.h, CAND) on
// tiles of 128 supports at every size; its query area holds the packed queries (B * d halves), half the width.
namespace {
struct KnnWs {
    CandOut cand;
    int64_t n_stiles;
    int kcp;
};
bool knn_shape_ok(int form, int64_t B, int64_t N, int64_t d, int64_t k) {
    // (d: the loaders' tile-relative offsets, as in plan_fused; half-precision rows: whole 64-k stages)
    const bool d_ok = form == FORM_HALF ? half_form_shape_ok(d) : form == FORM_SPLIT && d >= BK && d % BK == 0 && d <= (1 << 20);
    return B >= 0 && N > 25 && d_ok && k >= 1 && k <= 32 && k <= N && B < (1 << 30) && N < (1 << 30);
}
// BS: the tile height of the score-writing call of this shape; d: the width of a query-area row in floats
size_t knn_layout(int64_t B, int64_t N, int64_t d, int64_t k, int BS, char* base, KnnWs* out) {
    KnnWs w = {};   // (no row window)
    w.n_stiles = (N + BS - 1) / BS;
    w.kcp = cand_slots((int)k, BS);
    size_t off = 0;
    auto take = [&](size_t bytes) {
        char* p = base ? base + off : nullptr;
        off += al256(bytes);
        return p;
    };
    const size_t slots = (size_t)B * (size_t)w.n_stiles * (size_t)w.kcp;
    w.cand.key = reinterpret_cast<unsigned*>(take(slots * 4));
    w.cand.row = reinterpret_cast<int*>(take(slots * 4));
    w.cand.q_rows = reinterpret_cast<float*>(take((size_t)B * (size_t)d * 4));
    w.cand.q_scale = reinterpret_cast<float*>(take((size_t)B * 4));
    w.cand.q_norm2 = reinterpret_cast<float*>(take((size_t)B * 4));
    w.cand.k = (int)k;
    if (out) *out = w;
    return off;
}
size_t knn_layout(int form, int64_t B, int64_t N, int64_t d, int64_t k, char* base, KnnWs* out) {
    return knn_layout(B, N, form == FORM_HALF ? d / 2 : d, k, plan_tiles(B, N, d, form).BS, base, out);
}
}  // namespace

// What the call needs.  Half-precision rows: the layout of the shape.  Split rows: made non-decreasing in B, N and k: the
// tile height follows the shape (pick_rs), and a larger shape on taller tiles can need LESS than a smaller one on short
// tiles -- so the answer is the largest need over the shapes up to (B, N).  Only shapes below the large-grid rule of pick_rs
// (fewer than 1024 tiles of 128 rows: there the height is fixed and the need grows with the shape) have to be visited, one N
// per 16 rows and one B per 64 queries.  (The height rule alone is asked here, ~10^5 times for a large shape: no plans.)
size_t knn_workspace_bytes(int form, int64_t B, int64_t N, int64_t d, int64_t k) {
    if (!knn_shape_ok(form, B, N, d, k) || B == 0) return 0;
    if (form == FORM_HALF) return knn_layout(form, B, N, d, k, nullptr, nullptr);
    if (pick_rs(B, N, d, true) > 10) return 0;   // (the tile_rs knob at 12: no candidate form, plan_fused refuses)
    size_t need = knn_layout(B, N, d, k, 16 * pick_rs(B, N, d, true), nullptr, nullptr);
    const int64_t nq = (B + BQ - 1) / BQ;
    for (int64_t qt = 1; qt <= nq && qt < 1024; ++qt) {
        const int64_t Bq = qt * BQ < B ? qt * BQ : B;
        for (int64_t n = 17; n <= N && qt * ((n + 127) / 128) < 1024; n += 16) {   // n: the least N of its 16 rows
            const int64_t nn = n > 26 ? n : 26;
            if (nn > N || k > nn) continue;
            const size_t x = knn_layout(Bq, nn, d, k, 16 * pick_rs(Bq, nn, d, true), nullptr, nullptr);
            need = x > need ? x : need;
        }
    }
    return need;
}

int launch_knn(const KnnCall& c) {
    const bool window = c.row_lo != nullptr && c.row_hi != nullptr;
    if (!knn_shape_ok(c.form, c.B, c.N, c.d, c.k)) return NW_ERR_UNSUPPORTED;
    if (window && c.form == FORM_HALF) return NW_ERR_UNSUPPORTED;   // (the 256-query kernel has no windowed candidate form)
    if (c.B == 0) return NW_OK;
    KnnWs w;
    const size_t need = knn_layout(c.form, c.B, c.N, c.d, c.k, static_cast<char*>(c.workspace), &w);
    if (!c.workspace || c.workspace_bytes < need) return NW_ERR_WORKSPACE;
    if (w.n_stiles * w.kcp >= (1ll << 31)) return NW_ERR_UNSUPPORTED;
    if (window) w.cand.win_lo = c.row_lo, w.cand.win_hi = c.row_hi, w.cand.win_exclude = c.exclude != 0;
    FusedArgs a = {};   // no labels (sy is null: no run tables), no outputs, no workspace but the CandOut
    a.q = c.q, a.s = static_cast<const float*>(c.s_rows), a.s_norm2 = c.s_norm2, a.s_scale = c.s_scale;
    a.ls = c.logit_scale_dev;
    a.B = (int)c.B, a.N = (int)c.N, a.d = (int)c.d, a.C = 1, a.st = c.st, a.cand = &w.cand;
    const int rc = launch_fused(a, c.form, c.kind);
    if (rc != NW_OK) return rc;
    // (a window can leave a query fewer than k rows: the selection pads)
    return launch_topk_candidates(w.cand.key, w.cand.row, c.idx, c.vals, c.B, w.n_stiles * w.kcp, c.k, c.st, window);
}

}  // namespace nw

extern "C" size_t nw_bank_tables_bytes(int64_t N) {
    if (N <= 0 || N > 0x7fffffffLL) return 0;
    return nw::bank_tables_layout((N + nw::BANK_BS - 1) / nw::BANK_BS, nullptr, nullptr);
}

extern "C" int nw_bank_tables_build(const int64_t* sy, int64_t N, int64_t C, void* tables, size_t tables_bytes,
                                    void* stream) {
    using namespace nw;
    if (N < 0 || C < 0 || N > 0x7fffffffLL || C > 0x7fffffffLL) return NW_ERR_INVALID_ARG;
    if (N == 0) return NW_OK;
    if (!sy || !tables || (reinterpret_cast<uintptr_t>(tables) & 15)) return NW_ERR_INVALID_ARG;
    const int64_t n_stiles = (N + BANK_BS - 1) / BANK_BS;
    FusedWs ws;
    if (tables_bytes < bank_tables_layout(n_stiles, static_cast<char*>(tables), &ws)) return NW_ERR_WORKSPACE;
    return launch_run_tables(ws, sy, (int)N, (int)C, (int)n_stiles, BANK_BS, static_cast<hipStream_t>(stream));
}

