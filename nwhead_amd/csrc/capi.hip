// capi.hip -- the extern "C" surface declared in include/nwhead_hip.h (gfx950 / MI355X only).
#include <cstddef>
#include <cstdlib>
#include <string.h>
#include "nw_internal.h"
#include "fused_plan.h"
#include "bwd_plan.h"

namespace {
inline bool bad_kind(int kind) { return kind < NW_SCORE_EUCLIDEAN || kind > NW_SCORE_CLIP; }
}  // namespace

// Below ~2e8 multiply-adds the fp32-MFMA path with cached norms was the shorter one while the split-fp16 path
// had a query-split launch in front (measured then: B=64 N=1000 d=512 19.7 vs 29.8 us; B=256 N=10000 d=512
// 36.1 vs 23.9 us).  nw_fwd_opts.force_split takes the split path at every size.
extern "C" int nw_scores_use_split(int64_t B, int64_t N, int64_t d);   // the size rule, for callers that must follow it
static bool split_pays(int64_t B, int64_t N, int64_t d) {
    return nw::fwd_opts().force_split || nw_scores_use_split(B, N, d) != 0;
}
// Whether a call with this bank takes the split operands: the bank has them, the shape fits them, they pay (or are
// forced), and both operands are aligned.
static bool takes_split(const float* q, const float* s_split, const float* s_scale, const float* s_norm2, int64_t B, int64_t N,
                        int64_t d) {
    return s_split && s_scale && s_norm2 && d % 32 == 0 && split_pays(B, N, d) &&
           ((reinterpret_cast<uintptr_t>(s_split) | reinterpret_cast<uintptr_t>(q)) & 15) == 0;
}

namespace nw {
namespace {
thread_local FwdOpts tl_fwd_opts;     // of the forward entry point this thread is inside (OptsGuard), defaults outside
int g_knobs[KNOB_COUNT];
bool g_knobs_init = [] { for (int& k : g_knobs) k = KNOB_UNSET; return true; }();
const char* const knob_names[KNOB_COUNT] = {
    "pvar", "qg", "tile_rs", "no_persistent", "split_queries", "bwd_no_mfma", "bwd_split",
    "xgemm_wgs", "split_lbits", "conv_max_wgs", "conv_skip_cfgs", "conv_force_cfg"};
}  // namespace
const FwdOpts& fwd_opts() { return tl_fwd_opts; }
int knob(int id) { return (id >= 0 && id < KNOB_COUNT) ? __atomic_load_n(&g_knobs[id], __ATOMIC_RELAXED) : KNOB_UNSET; }
}  // namespace nw

namespace {
struct OptsGuard {   // the call's options are visible to the launch code of this thread until the entry point returns
    nw::FwdOpts saved;
    explicit OptsGuard(const nw_fwd_opts* o) : saved(nw::tl_fwd_opts) {
        nw::FwdOpts f;
        // (a caller built against an older header passes a shorter struct: the fields it has are honoured, and its tables,
        //  whose label array is then unknown, are not used)
        if (o && o->struct_size >= offsetof(nw_fwd_opts, tables)) {
            f.persistent_wgs = o->persistent_wgs;
            f.force_split = o->force_split;
            f.operand_form = o->operand_form;
        }
        if (o && o->struct_size >= sizeof(nw_fwd_opts)) {
            f.tables = static_cast<const char*>(o->tables);
            f.tables_bytes = o->tables_bytes;
            f.tables_sy = o->tables_sy;
            f.tables_N = o->tables_N;
        }
        nw::tl_fwd_opts = f;
    }
    ~OptsGuard() { nw::tl_fwd_opts = saved; }
};
}  // namespace

// nw_fwd_opts.operand_form = 1 (half-precision rows of nw_pack_rows_f16 in s_split): what the call must look like, checked
// before anything is launched.  NW_OK: take the FORM_HALF launch.
static int half_form_check(const float* q, const float* s, const float* s_norm2, const float* s_split, const float* s_scale,
                           const void* per_pair_out, int batched, int64_t B, int64_t N, int64_t d, int64_t C) {
    if (per_pair_out || batched) return NW_ERR_UNSUPPORTED;          // scores / weights, per-query supports or labels
    if (!nw::half_form_shape_ok(d)) return NW_ERR_UNSUPPORTED;
    if (B == 0 || N == 0 || C == 0) return NW_OK;                    // nothing to multiply: the common code answers
    if (!s_split || !s_scale || !s_norm2) return NW_ERR_INVALID_ARG;
    if ((reinterpret_cast<uintptr_t>(s_split) | reinterpret_cast<uintptr_t>(q)) & 15) return NW_ERR_INVALID_ARG;
    if (!nw::fused_eligible(q, s_split, B, N, d, C)) return NW_ERR_UNSUPPORTED;   // N <= 25, sizes past the tile kernels
    (void)s;
    return NW_OK;
}

extern "C" int nw_debug_set(const char* name, int value) {
    if (!name) return NW_ERR_INVALID_ARG;
    for (int k = 0; k < nw::KNOB_COUNT; ++k)
        if (!strcmp(name, nw::knob_names[k])) {
            __atomic_store_n(&nw::g_knobs[k], value, __ATOMIC_RELAXED);
            return NW_OK;
        }
    return NW_ERR_INVALID_ARG;
}

extern "C" int nw_debug_fwd_plan(int64_t B, int64_t N, int64_t d, int64_t C, int form, int outputs, int k, int norms, int kind,
                                 int persistent_wgs, int cus, nw_fwd_plan* plan) {
    if (!plan || B < 0 || N < 0 || d < 0 || C < 0 || k < 0 || cus < 0 || cus > (1 << 20)) return NW_ERR_INVALID_ARG;
    if (form < nw::FORM_F32 || form > nw::FORM_HALF || outputs < nw::OUT_NONE || outputs > nw::OUT_CAND) return NW_ERR_INVALID_ARG;
    if (bad_kind(kind)) return NW_ERR_UNSUPPORTED;
    nw::FwdOpts o;
    o.persistent_wgs = persistent_wgs;
    const nw::FusedPlan p = nw::plan_fused(B, N, d, C, form, outputs, k, norms != 0, kind == NW_SCORE_DOT, cus, o);
    *plan = {p.status, p.rs, p.BS, p.n_stiles, p.n_qtiles, p.grid, p.mode, p.out, p.dma, p.persistent, p.variant, p.workgroups,
             p.qgroup, p.split_queries, p.run_tables, 0, (uint64_t)p.lds_bytes};
    return NW_OK;
}

extern "C" int nw_abi_version(void) { return NW_ABI_VERSION; }

extern "C" const char* nw_status_string(int status) {
    switch (status) {
        case NW_OK: return "ok";
        case NW_ERR_INVALID_ARG: return "invalid argument";
        case NW_ERR_UNSUPPORTED: return "unsupported score kind or size";
        case NW_ERR_WORKSPACE: return "workspace too small";
        case NW_ERR_LAUNCH: return "HIP launch failed";
        case NW_ERR_NO_DEVICE: return "no gfx950 device";
        default: return "unknown status";
    }
}

extern "C" int nw_device_check(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return NW_ERR_NO_DEVICE;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return NW_ERR_NO_DEVICE;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return NW_ERR_NO_DEVICE;
    return strncmp(prop.gcnArchName, "gfx950", 6) == 0 ? NW_OK : NW_ERR_NO_DEVICE;
}

extern "C" int nw_scores_f32(const float* q, const float* s, float* scores, int64_t B, int64_t N,
                             int64_t d, int kind, const float* logit_scale_dev, int sup_batched,
                             void* stream) {
    if (B < 0 || N < 0 || d < 0) return NW_ERR_INVALID_ARG;
    if (bad_kind(kind)) return NW_ERR_UNSUPPORTED;
    if (B == 0 || N == 0) return NW_OK;
    if (!q || !s || !scores) return NW_ERR_INVALID_ARG;
    if (kind == NW_SCORE_CLIP && !logit_scale_dev) return NW_ERR_INVALID_ARG;
    return nw::launch_scores(q, s, scores, B, N, d, kind, logit_scale_dev, sup_batched,
                             static_cast<hipStream_t>(stream));
}

// Scratch: the fused path keeps per-tile softmax statistics and label-run sums (fused.hip); the
// two-kernel path (per-query supports, N <= 25, weights requested) one (B,N) score matrix.  nw::FwdLayout is the map.
extern "C" size_t nw_fwd_workspace_bytes(int64_t B, int64_t N, int64_t d, int64_t C) {
    return nw::fwd_layout(B, N, d, C, nullptr).total;
}

extern "C" int nw_debug_fwd_layout(int64_t B, int64_t N, int64_t d, int64_t C, nw_fwd_layout* layout) {
    if (!layout || B < 0 || N < 0 || d < 0 || C < 0) return NW_ERR_INVALID_ARG;
    const nw::FwdLayout L = nw::fwd_layout(B, N, d, C, nullptr);
    const nw::FwdLayout::Area* const areas[NW_FWD_AREAS] = {&L.main, &L.q_rows, &L.q_scale, &L.q_norm2, &L.lse, &L.slices};
    *layout = {};
    for (int i = 0; i < NW_FWD_AREAS; ++i) layout->off[i] = areas[i]->off, layout->bytes[i] = areas[i]->bytes;
    layout->total = L.total;
    layout->n_slices = L.n_slices;
    return NW_OK;
}

extern "C" int nw_debug_bwd_plan(int64_t B, int64_t N, int64_t d, int64_t C, int sup_batched, nw_bwd_plan* plan) {
    static_assert(NW_BWD_AREAS == nw::BWD_AREAS, "nw_bwd_plan lists the areas of nw::BwdPlan");
    if (!plan || B < 0 || N < 0 || d < 0 || C < 0) return NW_ERR_INVALID_ARG;
    const nw::BwdPlan p = nw::plan_bwd(B, N, d, C, sup_batched);
    *plan = {};
    plan->status = p.status, plan->route = p.route, plan->coeff_threads = (int32_t)p.coeff_threads, plan->parts_shared = p.parts_shared;
    plan->gq_chunks = p.gq.nchunks, plan->gq_k_chunk = p.gq.k_chunk, plan->gs_chunks = p.gs.nchunks, plan->gs_k_chunk = p.gs.k_chunk;
    plan->ld = p.ld, plan->Bpad = p.Bpad, plan->coeff_lds_bytes = p.coeff_lds, plan->total = p.total;
    for (int i = 0; i < NW_BWD_AREAS; ++i) plan->off[i] = p.area[i].off, plan->bytes[i] = p.area[i].bytes;
    return NW_OK;
}

extern "C" int nw_row_norm2_f32(const float* x, float* n2, int64_t rows, int64_t d, void* stream) {
    if (rows < 0 || d < 0) return NW_ERR_INVALID_ARG;
    if (rows == 0) return NW_OK;
    if (!x || !n2) return NW_ERR_INVALID_ARG;
    return nw::launch_rownorm2(x, n2, rows, d, static_cast<hipStream_t>(stream));
}

// nw_fwd_f32 inside its options guard.  carved: the workspace as an entry point that has checked the shape already carved it
// (nw_fwd_influence_f32), or null.
static int fwd_f32(const float* q, const float* s, const int64_t* sy, const float* s_norm2, const float* s_split,
                   const float* s_scale, float* out, float* scores_out, float* lse_out, float* weights_out, void* workspace,
                   size_t workspace_bytes, const nw::FwdLayout* carved, int64_t B, int64_t N, int64_t d, int64_t C, int kind,
                   const float* logit_scale_dev, int sup_batched, int labels_batched, hipStream_t st) {
    if (B < 0 || N < 0 || d < 0 || C < 0) return NW_ERR_INVALID_ARG;
    if (bad_kind(kind)) return NW_ERR_UNSUPPORTED;
    if (B == 0) return NW_OK;
    if (!out && C > 0) return NW_ERR_INVALID_ARG;
    if (N > 0 && (!q || !s || !sy)) return NW_ERR_INVALID_ARG;
    if (kind == NW_SCORE_CLIP && !logit_scale_dev) return NW_ERR_INVALID_ARG;
    if (labels_batched && !sup_batched) return NW_ERR_INVALID_ARG;
    const int form = nw::fwd_opts().operand_form;
    if (form != 0 && form != 1) return NW_ERR_INVALID_ARG;
    const nw::FwdLayout L = carved ? *carved : nw::fwd_layout(B, N, d, C, workspace);
    // the fused launch's operands: fp32 supports; the split / half-precision routes below swap the bank's rows in
    nw::FusedArgs a = {q, s, sy, s_norm2, nullptr, logit_scale_dev, out, scores_out, lse_out, nullptr, nullptr, nullptr,
                       &L, (int)B, (int)N, (int)d, (int)C, st, nullptr};
    if (form == 1) {
        const int rc = half_form_check(q, s, s_norm2, s_split, s_scale, scores_out ? scores_out : weights_out,
                                       sup_batched || labels_batched, B, N, d, C);
        if (rc != NW_OK) return rc;
        if (N > 0 && C > 0) {
            if (!L.fits(workspace_bytes)) return NW_ERR_WORKSPACE;
            a.s = s_split, a.s_scale = s_scale;
            return nw::launch_fused(a, nw::FORM_HALF, kind);
        }
    }
    // Softmax weights on request: the fused kernel writes the scores where the weights go and one in-place pass
    // normalises them with the merge's log-sum-exp (w = exp(score - lse), the workspace's lse area when the caller asks
    // for none); the two-kernel fallback below streams the (B,N) matrix five times.
    float* sc_buf = scores_out ? scores_out : weights_out;
    if (N > 0 && C > 0 && !sup_batched && nw::fused_eligible(q, s, B, N, d, C) &&
        (!sc_buf || (reinterpret_cast<uintptr_t>(sc_buf) & 15) == 0)) {
        if (!L.fits(workspace_bytes)) return NW_ERR_WORKSPACE;
        a.scores = sc_buf;
        if (weights_out && !a.lse) a.lse = L.at(L.lse);
        const bool split = takes_split(q, s_split, s_scale, s_norm2, B, N, d);
        if (split) a.s = s_split, a.s_scale = s_scale;
        const int rc = nw::launch_fused(a, split ? nw::FORM_SPLIT : nw::FORM_F32, kind);
        if (rc != NW_OK || !weights_out) return rc;
        return nw::launch_weights_from_scores(sc_buf, a.lse, weights_out, B, N, st);
    }
    float* scores = scores_out;
    if (!scores && N > 0) {
        if (!L.fits(workspace_bytes)) return NW_ERR_WORKSPACE;
        scores = L.at(L.main);
    }
    int rc = nw::launch_scores(q, s, scores, B, N, d, kind, logit_scale_dev, sup_batched, st);
    if (rc != NW_OK) return rc;
    const bool sliced = L.n_slices > 1 && L.fits(workspace_bytes);
    return nw::launch_aggregate(scores, sy, labels_batched, out, lse_out, weights_out, nullptr, nullptr, nullptr, B, N, C, st,
                                sliced ? L.at(L.slices) : nullptr, sliced ? L.slices.bytes / sizeof(float) : 0);
}

extern "C" int nw_fwd_f32(const float* q, const float* s, const int64_t* sy, const float* s_norm2,
                          const float* s_split, const float* s_scale, float* out, float* scores_out, float* lse_out, float* weights_out, void* workspace,
                          size_t workspace_bytes, int64_t B, int64_t N, int64_t d, int64_t C,
                          int kind, const float* logit_scale_dev, int sup_batched,
                          int labels_batched, const nw_fwd_opts* opts, void* stream) {
    OptsGuard opts_guard(opts);
    return fwd_f32(q, s, sy, s_norm2, s_split, s_scale, out, scores_out, lse_out, weights_out, workspace, workspace_bytes, nullptr,
                   B, N, d, C, kind, logit_scale_dev, sup_batched, labels_batched, static_cast<hipStream_t>(stream));
}

// The head over a resident split bank and its gradients (fused.hip OUT_WIN / OUT_WGT, bwd_query.hip WGT / GA): one argument
// rule for the two forward entries and one for the three backward ones.  An entry builds its call record and names the
// optional operands it REQUIRES; the order of the checks, which decides the status of a call with several faults, is here.
// The regime of all five, stated here and nowhere else (bwd_query_shape_ok adds the integer ranges of the backward's index
// arithmetic; the forward leaves its own to fused_eligible, asked after B == 0 has answered):
bool nw::bank_head_shape_ok(int64_t N, int64_t d, int64_t C) { return N > 25 && C >= 1 && d >= 32 && d % 32 == 0 && d <= (1 << 20); }

namespace {
enum { NEED_WINDOW = 1, NEED_LOGW = 2, NEED_GQ = 4, NEED_GLOGW = 8 };
inline uintptr_t addr(const void* p) { return reinterpret_cast<uintptr_t>(p); }

// The forward: nw_fwd_f32's workspace, no options (nothing of nw_fwd_opts applies: split rows at every size, no run tables,
// no persistent kernel).  row_logw is read in float4s from row offsets that are multiples of four: 16-byte aligned
struct BankFwdCall {
    const float *q, *s_split, *s_scale, *s_norm2;
    const int64_t* sy;
    const float* row_logw;            // or null
    const int32_t *row_lo, *row_hi;   // both or neither; exclude reaches the kernel only with them
    int exclude;
    float *out, *lse_out;
    void* workspace;
    size_t workspace_bytes;
    int64_t B, N, d, C;
    int kind;
    const float* logit_scale_dev;
    void* stream;
};
int bank_fwd_checked(const BankFwdCall& c, int needs) {
    if (c.B < 0 || c.N < 0 || c.d < 0 || c.C < 0) return NW_ERR_INVALID_ARG;
    if ((c.row_lo != nullptr) != (c.row_hi != nullptr) || ((needs & NEED_WINDOW) && !c.row_lo)) return NW_ERR_INVALID_ARG;
    if (bad_kind(c.kind)) return NW_ERR_UNSUPPORTED;
    if (!nw::bank_head_shape_ok(c.N, c.d, c.C)) return NW_ERR_UNSUPPORTED;
    if (c.B == 0) return NW_OK;       // before any pointer is looked at
    if (!c.q || !c.s_split || !c.s_scale || !c.s_norm2 || !c.sy || !c.out || ((needs & NEED_LOGW) && !c.row_logw))
        return NW_ERR_INVALID_ARG;
    if (c.kind == NW_SCORE_CLIP && !c.logit_scale_dev) return NW_ERR_INVALID_ARG;
    if (!nw::fused_eligible(c.q, c.s_split, c.B, c.N, c.d, c.C)) return NW_ERR_UNSUPPORTED;   // alignment, sizes past the tile kernels
    if (addr(c.row_logw) & 15) return NW_ERR_UNSUPPORTED;
    const nw::FwdLayout L = nw::fwd_layout(c.B, c.N, c.d, c.C, c.workspace);
    if (!L.fits(c.workspace_bytes)) return NW_ERR_WORKSPACE;
    if (addr(c.workspace) & 15) return NW_ERR_UNSUPPORTED;
    nw::FusedArgs a = {c.q, c.s_split, c.sy, c.s_norm2, c.s_scale, c.logit_scale_dev, c.out, nullptr, c.lse_out, nullptr, nullptr,
                       nullptr, &L, (int)c.B, (int)c.N, (int)c.d, (int)c.C, static_cast<hipStream_t>(c.stream), nullptr,
                       c.row_lo, c.row_hi, c.row_lo && c.exclude != 0, c.row_logw};
    return nw::launch_fused(a, nw::FORM_SPLIT, c.kind);
}

// The backward, over the launcher's own record: a null gq / glogw / row_logw adds nothing to the alignment test; with glogw
// the workspace is the weights' (smaller without gq)
int bank_bwd_checked(const nw::BwdQueryCall& c, int needs) {
    if (c.B < 0 || c.N < 0 || c.d < 0 || c.C < 0 || c.row_chunks < 0) return NW_ERR_INVALID_ARG;
    if ((c.row_lo != nullptr) != (c.row_hi != nullptr)) return NW_ERR_INVALID_ARG;
    if (bad_kind(c.kind)) return NW_ERR_UNSUPPORTED;
    if (!nw::bwd_query_shape_ok(c.B, c.N, c.d, c.C)) return NW_ERR_UNSUPPORTED;
    if (c.B == 0) return NW_OK;       // before any pointer is looked at: nothing is touched, glogw included
    if (!c.q || !c.s_split || !c.s_scale || !c.s_norm2 || !c.sy || !c.lse || !c.out || !c.gout ||
        ((needs & NEED_LOGW) && !c.row_logw) || ((needs & NEED_GQ) && !c.gq) || ((needs & NEED_GLOGW) && !c.glogw))
        return NW_ERR_INVALID_ARG;
    if (c.kind == NW_SCORE_CLIP && !c.logit_scale_dev) return NW_ERR_INVALID_ARG;
    if ((addr(c.q) | addr(c.s_split) | addr(c.gq) | addr(c.row_logw) | addr(c.glogw)) & 15) return NW_ERR_UNSUPPORTED;
    const size_t need = c.glogw ? nw::bwd_logw_workspace_bytes(c.B, c.N, c.d, c.C, c.row_chunks, c.gq != nullptr)
                                : nw::bwd_query_workspace_bytes(c.B, c.N, c.d, c.C, c.row_chunks);
    if (!c.workspace || c.workspace_bytes < need) return NW_ERR_WORKSPACE;
    if (addr(c.workspace) & 15) return NW_ERR_UNSUPPORTED;
    return nw::launch_bwd_query(c);
}
}  // namespace

extern "C" int nw_fwd_window_f32(const float* q, const float* s_split, const float* s_scale, const float* s_norm2,
                                 const int64_t* sy, const int32_t* row_lo, const int32_t* row_hi, int exclude, float* out,
                                 float* lse_out, void* workspace, size_t workspace_bytes, int64_t B, int64_t N, int64_t d,
                                 int64_t C, int kind, const float* logit_scale_dev, void* stream) {
    return bank_fwd_checked({q, s_split, s_scale, s_norm2, sy, nullptr, row_lo, row_hi, exclude, out, lse_out, workspace,
                             workspace_bytes, B, N, d, C, kind, logit_scale_dev, stream}, NEED_WINDOW);
}

extern "C" int nw_fwd_weighted_f32(const float* q, const float* s_split, const float* s_scale, const float* s_norm2,
                                   const int64_t* sy, const float* row_logw, const int32_t* row_lo, const int32_t* row_hi,
                                   int exclude, float* out, float* lse_out, void* workspace, size_t workspace_bytes, int64_t B,
                                   int64_t N, int64_t d, int64_t C, int kind, const float* logit_scale_dev, void* stream) {
    return bank_fwd_checked({q, s_split, s_scale, s_norm2, sy, row_logw, row_lo, row_hi, exclude, out, lse_out, workspace,
                             workspace_bytes, B, N, d, C, kind, logit_scale_dev, stream}, NEED_LOGW);
}

extern "C" size_t nw_bwd_query_workspace_bytes(int64_t B, int64_t N, int64_t d, int64_t C, int row_chunks) {
    if (B <= 0 || N < 0 || d < 0 || C < 0) return 0;
    return nw::bwd_query_workspace_bytes(B, N, d, C, row_chunks);
}

extern "C" size_t nw_bwd_logw_workspace_bytes(int64_t B, int64_t N, int64_t d, int64_t C, int row_chunks, int want_gq) {
    if (B <= 0 || N < 0 || d < 0 || C < 0) return 0;
    return nw::bwd_logw_workspace_bytes(B, N, d, C, row_chunks, want_gq != 0);
}

extern "C" int nw_bwd_query_f32(const float* q, const float* s_split, const float* s_scale, const float* s_norm2,
                                const int64_t* sy, const int32_t* row_lo, const int32_t* row_hi, int exclude,
                                const float* lse, const float* out, const float* gout, float* gq, float* glogit_scale,
                                void* workspace, size_t workspace_bytes, int64_t B, int64_t N, int64_t d, int64_t C,
                                int kind, const float* logit_scale_dev, int row_chunks, void* stream) {
    return bank_bwd_checked({q, s_split, s_scale, s_norm2, sy, row_lo, row_hi, exclude, lse, out, gout, gq, glogit_scale,
                             workspace, workspace_bytes, B, N, d, C, kind, logit_scale_dev, row_chunks,
                             static_cast<hipStream_t>(stream), nullptr, nullptr}, NEED_GQ);
}

extern "C" int nw_bwd_query_weighted_f32(const float* q, const float* s_split, const float* s_scale, const float* s_norm2,
                                         const int64_t* sy, const float* row_logw, const int32_t* row_lo, const int32_t* row_hi,
                                         int exclude, const float* lse, const float* out, const float* gout, float* gq,
                                         float* glogit_scale, void* workspace, size_t workspace_bytes, int64_t B, int64_t N,
                                         int64_t d, int64_t C, int kind, const float* logit_scale_dev, int row_chunks,
                                         void* stream) {
    return bank_bwd_checked({q, s_split, s_scale, s_norm2, sy, row_lo, row_hi, exclude, lse, out, gout, gq, glogit_scale,
                             workspace, workspace_bytes, B, N, d, C, kind, logit_scale_dev, row_chunks,
                             static_cast<hipStream_t>(stream), row_logw, nullptr}, NEED_LOGW | NEED_GQ);
}

extern "C" int nw_bwd_query_logw_f32(const float* q, const float* s_split, const float* s_scale, const float* s_norm2,
                                     const int64_t* sy, const float* row_logw, const int32_t* row_lo, const int32_t* row_hi,
                                     int exclude, const float* lse, const float* out, const float* gout, float* gq, float* glogw,
                                     float* glogit_scale, void* workspace, size_t workspace_bytes, int64_t B, int64_t N,
                                     int64_t d, int64_t C, int kind, const float* logit_scale_dev, int row_chunks, void* stream) {
    return bank_bwd_checked({q, s_split, s_scale, s_norm2, sy, row_lo, row_hi, exclude, lse, out, gout, gq, glogit_scale,
                             workspace, workspace_bytes, B, N, d, C, kind, logit_scale_dev, row_chunks,
                             static_cast<hipStream_t>(stream), row_logw, glogw}, NEED_LOGW | NEED_GLOGW);
}

// The value head over the same bank (fwd_values.hip): the argument rule of the backward entries above, in their order, with
// the value rows in the labels' place and T in C's.
extern "C" size_t nw_fwd_values_workspace_bytes(int64_t B, int64_t N, int64_t d, int64_t T, int row_chunks) {
    if (B <= 0 || N < 0 || d < 0 || T < 0 || row_chunks < 0) return 0;
    return nw::fwd_values_workspace_bytes(B, N, d, T, row_chunks);
}

extern "C" int nw_fwd_values_f32(const float* q, const float* s_split, const float* s_scale, const float* s_norm2,
                                 const float* v_split, const float* v_scale, const float* row_logw, const int32_t* row_lo,
                                 const int32_t* row_hi, int exclude, const float* lse, float* out, void* workspace,
                                 size_t workspace_bytes, int64_t B, int64_t N, int64_t d, int64_t T, int kind,
                                 const float* logit_scale_dev, int row_chunks, void* stream) {
    if (B < 0 || N < 0 || d < 0 || T < 0 || row_chunks < 0) return NW_ERR_INVALID_ARG;
    if ((row_lo != nullptr) != (row_hi != nullptr)) return NW_ERR_INVALID_ARG;
    if (bad_kind(kind)) return NW_ERR_UNSUPPORTED;
    if (!nw::fwd_values_shape_ok(B, N, d, T)) return NW_ERR_UNSUPPORTED;
    if (B == 0) return NW_OK;         // before any pointer is looked at
    if (!q || !s_split || !s_scale || !s_norm2 || !v_split || !v_scale || !lse || !out) return NW_ERR_INVALID_ARG;
    if (kind == NW_SCORE_CLIP && !logit_scale_dev) return NW_ERR_INVALID_ARG;
    if ((addr(q) | addr(s_split) | addr(v_split) | addr(out) | addr(row_logw)) & 15) return NW_ERR_UNSUPPORTED;
    const size_t need = nw::fwd_values_workspace_bytes(B, N, d, T, row_chunks);
    if (!workspace || workspace_bytes < need) return NW_ERR_WORKSPACE;
    if (addr(workspace) & 15) return NW_ERR_UNSUPPORTED;
    return nw::launch_fwd_values({q, s_split, s_scale, s_norm2, v_split, v_scale, row_logw, row_lo, row_hi, exclude, lse, out,
                                  workspace, workspace_bytes, B, N, d, T, kind, logit_scale_dev, row_chunks,
                                  static_cast<hipStream_t>(stream)});
}

// ... and its gradient w.r.t. the queries (bwd_values.hip): nw_fwd_values_f32's rule with the backward's operands.
extern "C" size_t nw_bwd_values_query_workspace_bytes(int64_t B, int64_t N, int64_t d, int64_t T, int row_chunks) {
    if (B <= 0 || N < 0 || d < 0 || T < 0 || row_chunks < 0) return 0;
    return nw::bwd_values_workspace_bytes(B, N, d, T, row_chunks);
}

extern "C" int nw_bwd_values_query_f32(const float* q, const float* s_split, const float* s_scale, const float* s_norm2,
                                       const float* v_split, const float* v_scale, const float* row_logw, const int32_t* row_lo,
                                       const int32_t* row_hi, int exclude, const float* lse, const float* out, const float* gout,
                                       float* gq, float* glogit_scale, void* workspace, size_t workspace_bytes, int64_t B,
                                       int64_t N, int64_t d, int64_t T, int kind, const float* logit_scale_dev, int row_chunks,
                                       void* stream) {
    if (B < 0 || N < 0 || d < 0 || T < 0 || row_chunks < 0) return NW_ERR_INVALID_ARG;
    if ((row_lo != nullptr) != (row_hi != nullptr)) return NW_ERR_INVALID_ARG;
    if (bad_kind(kind)) return NW_ERR_UNSUPPORTED;
    if (!nw::bwd_values_shape_ok(B, N, d, T)) return NW_ERR_UNSUPPORTED;
    if (B == 0) return NW_OK;         // before any pointer is looked at
    if (!q || !s_split || !s_scale || !s_norm2 || !v_split || !v_scale || !lse || !out || !gout || !gq) return NW_ERR_INVALID_ARG;
    if (kind == NW_SCORE_CLIP && !logit_scale_dev) return NW_ERR_INVALID_ARG;
    if ((addr(q) | addr(s_split) | addr(v_split) | addr(gout) | addr(gq) | addr(row_logw)) & 15) return NW_ERR_UNSUPPORTED;
    const size_t need = nw::bwd_values_workspace_bytes(B, N, d, T, row_chunks);
    if (!workspace || workspace_bytes < need) return NW_ERR_WORKSPACE;
    if (addr(workspace) & 15) return NW_ERR_UNSUPPORTED;
    return nw::launch_bwd_values({q, s_split, s_scale, s_norm2, v_split, v_scale, row_logw, row_lo, row_hi, exclude, lse, out,
                                  gout, gq, glogit_scale, workspace, workspace_bytes, B, N, d, T, kind, logit_scale_dev,
                                  row_chunks, static_cast<hipStream_t>(stream)});
}

// ... and w.r.t. the values and the row weights (bwd_values_support.hip): the same rule; the fp32 value rows and the weights
// are required with glogw only.
extern "C" size_t nw_bwd_values_support_workspace_bytes(int64_t B, int64_t N, int64_t d, int64_t T, int query_chunks,
                                                        int want_gvalues) {
    if (B <= 0 || N < 0 || d < 0 || T < 0 || query_chunks < 0) return 0;
    return nw::bwd_values_support_workspace_bytes(B, N, d, T, query_chunks, want_gvalues != 0);
}

extern "C" int nw_bwd_values_support_f32(const float* q, const float* s_split, const float* s_scale, const float* s_norm2,
                                         const float* v_rows, const float* row_logw, const int32_t* row_lo, const int32_t* row_hi,
                                         int exclude, const float* lse, const float* out, const float* gout, float* gvalues,
                                         float* glogw, void* workspace, size_t workspace_bytes, int64_t B, int64_t N, int64_t d,
                                         int64_t T, int kind, const float* logit_scale_dev, int query_chunks, void* stream) {
    if (B < 0 || N < 0 || d < 0 || T < 0 || query_chunks < 0) return NW_ERR_INVALID_ARG;
    if ((row_lo != nullptr) != (row_hi != nullptr)) return NW_ERR_INVALID_ARG;
    if (bad_kind(kind)) return NW_ERR_UNSUPPORTED;
    if (!nw::fwd_values_shape_ok(B, N, d, T)) return NW_ERR_UNSUPPORTED;
    if (B == 0) return NW_OK;         // before any pointer is looked at: nothing is touched, gvalues and glogw included
    if (!q || !s_split || !s_scale || !s_norm2 || !lse || !out || !gout || (!gvalues && !glogw)) return NW_ERR_INVALID_ARG;
    if (glogw && (!row_logw || !v_rows)) return NW_ERR_INVALID_ARG;
    if (kind == NW_SCORE_CLIP && !logit_scale_dev) return NW_ERR_INVALID_ARG;
    if ((addr(q) | addr(s_split) | addr(v_rows) | addr(gout) | addr(gvalues) | addr(glogw) | addr(row_logw)) & 15)
        return NW_ERR_UNSUPPORTED;
    const size_t need = nw::bwd_values_support_workspace_bytes(B, N, d, T, query_chunks, gvalues != nullptr);
    if (!workspace || workspace_bytes < need) return NW_ERR_WORKSPACE;
    if (addr(workspace) & 15) return NW_ERR_UNSUPPORTED;
    return nw::launch_bwd_values_support({q, s_split, s_scale, s_norm2, v_rows, row_logw, row_lo, row_hi, exclude, lse, out, gout,
                                          gvalues, glogw, workspace, workspace_bytes, B, N, d, T, kind, logit_scale_dev,
                                          query_chunks, static_cast<hipStream_t>(stream)});
}

// The class head's gradient w.r.t. the bank rows (bwd_support.hip): the backward entries' rule above, in their order, with
// the fp32 rows and gs required.
extern "C" size_t nw_bwd_bank_support_workspace_bytes(int64_t B, int64_t N, int64_t d, int64_t C, int query_chunks) {
    if (B <= 0 || N < 0 || d < 0 || C < 0 || query_chunks < 0) return 0;
    return nw::bwd_bank_support_workspace_bytes(B, N, d, C, query_chunks);
}

extern "C" int nw_bwd_bank_support_f32(const float* q, const float* s, const float* s_split, const float* s_scale,
                                       const float* s_norm2, const int64_t* sy, const float* row_logw, const int32_t* row_lo,
                                       const int32_t* row_hi, int exclude, const float* lse, const float* out, const float* gout,
                                       float* gs, void* workspace, size_t workspace_bytes, int64_t B, int64_t N, int64_t d,
                                       int64_t C, int kind, const float* logit_scale_dev, int query_chunks, void* stream) {
    if (B < 0 || N < 0 || d < 0 || C < 0 || query_chunks < 0) return NW_ERR_INVALID_ARG;
    if ((row_lo != nullptr) != (row_hi != nullptr)) return NW_ERR_INVALID_ARG;
    if (bad_kind(kind)) return NW_ERR_UNSUPPORTED;
    if (!nw::bwd_query_shape_ok(B, N, d, C)) return NW_ERR_UNSUPPORTED;
    if (B == 0) return NW_OK;         // before any pointer is looked at: nothing is touched, gs included
    if (!q || !s || !s_split || !s_scale || !s_norm2 || !sy || !lse || !out || !gout || !gs) return NW_ERR_INVALID_ARG;
    if (kind == NW_SCORE_CLIP && !logit_scale_dev) return NW_ERR_INVALID_ARG;
    if ((addr(q) | addr(s) | addr(s_split) | addr(gs) | addr(row_logw)) & 15) return NW_ERR_UNSUPPORTED;
    const size_t need = nw::bwd_bank_support_workspace_bytes(B, N, d, C, query_chunks);
    if (!workspace || workspace_bytes < need) return NW_ERR_WORKSPACE;
    if (addr(workspace) & 15) return NW_ERR_UNSUPPORTED;
    return nw::launch_bwd_bank_support({q, s, s_split, s_scale, s_norm2, sy, row_logw, row_lo, row_hi, exclude, lse, out, gout, gs,
                                        workspace, workspace_bytes, B, N, d, C, kind, logit_scale_dev, query_chunks,
                                        static_cast<hipStream_t>(stream)});
}

// The value head's gradient w.r.t. the bank rows (bwd_values_bank.hip): nw_bwd_values_support_f32's rule, in its order, with
// nw_bwd_bank_support_f32's for the fp32 rows and gs.
extern "C" size_t nw_bwd_values_bank_support_workspace_bytes(int64_t B, int64_t N, int64_t d, int64_t T, int query_chunks) {
    if (B <= 0 || N < 0 || d < 0 || T < 0 || query_chunks < 0) return 0;
    return nw::bwd_values_bank_support_workspace_bytes(B, N, d, T, query_chunks);
}

extern "C" int nw_bwd_values_bank_support_f32(const float* q, const float* s, const float* s_split, const float* s_scale,
                                              const float* s_norm2, const float* v_split, const float* v_scale,
                                              const float* row_logw, const int32_t* row_lo, const int32_t* row_hi, int exclude,
                                              const float* lse, const float* out, const float* gout, float* gs, void* workspace,
                                              size_t workspace_bytes, int64_t B, int64_t N, int64_t d, int64_t T, int kind,
                                              const float* logit_scale_dev, int query_chunks, void* stream) {
    if (B < 0 || N < 0 || d < 0 || T < 0 || query_chunks < 0) return NW_ERR_INVALID_ARG;
    if ((row_lo != nullptr) != (row_hi != nullptr)) return NW_ERR_INVALID_ARG;
    if (bad_kind(kind)) return NW_ERR_UNSUPPORTED;
    if (!nw::fwd_values_shape_ok(B, N, d, T)) return NW_ERR_UNSUPPORTED;
    if (B == 0) return NW_OK;         // before any pointer is looked at: nothing is touched, gs included
    if (!q || !s || !s_split || !s_scale || !s_norm2 || !v_split || !v_scale || !lse || !out || !gout || !gs)
        return NW_ERR_INVALID_ARG;
    if (kind == NW_SCORE_CLIP && !logit_scale_dev) return NW_ERR_INVALID_ARG;
    if ((addr(q) | addr(s) | addr(s_split) | addr(v_split) | addr(gout) | addr(gs) | addr(row_logw)) & 15) return NW_ERR_UNSUPPORTED;
    const size_t need = nw::bwd_values_bank_support_workspace_bytes(B, N, d, T, query_chunks);
    if (!workspace || workspace_bytes < need) return NW_ERR_WORKSPACE;
    if (addr(workspace) & 15) return NW_ERR_UNSUPPORTED;
    return nw::launch_bwd_values_bank_support({q, s, s_split, s_scale, s_norm2, v_split, v_scale, row_logw, row_lo, row_hi, exclude,
                                               lse, out, gout, gs, workspace, workspace_bytes, B, N, d, T, kind, logit_scale_dev,
                                               query_chunks, static_cast<hipStream_t>(stream)});
}

extern "C" int nw_fwd_partial_f32(const float* q, const float* s, const int64_t* sy,
                                  const float* s_norm2, const float* s_split, const float* s_scale,
                                  float* m, float* den, float* num, void* workspace, size_t workspace_bytes,
                                  int64_t B, int64_t N, int64_t d, int64_t C, int kind,
                                  const float* logit_scale_dev, const nw_fwd_opts* opts, void* stream) {
    OptsGuard opts_guard(opts);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (B < 0 || N < 0 || d < 0 || C < 0) return NW_ERR_INVALID_ARG;
    if (bad_kind(kind)) return NW_ERR_UNSUPPORTED;
    if (B == 0) return NW_OK;
    if (!m || !den || (!num && C > 0)) return NW_ERR_INVALID_ARG;
    if (N > 0 && (!q || !s || !sy)) return NW_ERR_INVALID_ARG;
    if (kind == NW_SCORE_CLIP && !logit_scale_dev) return NW_ERR_INVALID_ARG;
    const int form = nw::fwd_opts().operand_form;
    if (form != 0 && form != 1) return NW_ERR_INVALID_ARG;
    if (form == 1) {
        const int rc = half_form_check(q, s, s_norm2, s_split, s_scale, nullptr, 0, B, N, d, C);
        if (rc != NW_OK) return rc;
    }
    const nw::FwdLayout L = nw::fwd_layout(B, N, d, C, workspace);
    if (N > 0 && !L.fits(workspace_bytes)) return NW_ERR_WORKSPACE;
    nw::FusedArgs a = {q, s, sy, s_norm2, nullptr, logit_scale_dev, nullptr, nullptr, nullptr, m, den, num,
                       &L, (int)B, (int)N, (int)d, (int)C, st, nullptr};
    if (form == 1 && N > 0 && C > 0) {
        a.s = s_split, a.s_scale = s_scale;
        return nw::launch_fused(a, nw::FORM_HALF, kind);
    }
    if (N > 0 && C > 0 && nw::fused_eligible(q, s, B, N, d, C)) {
        if (!takes_split(q, s_split, s_scale, s_norm2, B, N, d)) return nw::launch_fused(a, nw::FORM_F32, kind);
        a.s = s_split, a.s_scale = s_scale;
        return nw::launch_fused(a, nw::FORM_SPLIT, kind);
    }
    float* scores = L.at(L.main);
    int rc = nw::launch_scores(q, s, scores, B, N, d, kind, logit_scale_dev, 0, st);
    if (rc != NW_OK) return rc;
    return nw::launch_aggregate(scores, sy, 0, nullptr, nullptr, nullptr, m, den, num, B, N, C, st);
}

extern "C" int nw_merge_finalize_f32(const float* m, const float* den, const float* num, float* out,
                                     int64_t G, int64_t B, int64_t C, int64_t stride_m,
                                     int64_t stride_den, int64_t stride_num,
                                     const int64_t* class_lo, int64_t C_local, void* stream) {
    if (G < 0 || B < 0 || C < 0) return NW_ERR_INVALID_ARG;
    if (B == 0 || C == 0) return NW_OK;
    if (!m || !den || !num || !out) return NW_ERR_INVALID_ARG;
    if (class_lo && C_local <= 0) return NW_ERR_INVALID_ARG;
    return nw::launch_merge(m, den, num, out, G, B, C, stride_m, stride_den, stride_num, class_lo,
                            class_lo ? C_local : C, static_cast<hipStream_t>(stream));
}

extern "C" int nw_topk_f32(const float* scores, int64_t* idx_out, float* val_out, int64_t B, int64_t N, int64_t k,
                           void* stream) {
    if (B < 0 || N < 0 || (B > 0 && (!scores || !idx_out))) return NW_ERR_INVALID_ARG;
    return nw::launch_topk(scores, idx_out, val_out, B, N, k, static_cast<hipStream_t>(stream));
}

extern "C" int nw_scores_use_split(int64_t B, int64_t N, int64_t d) {
    return B > 0 && N > 0 && d > 0 && (double)B * (double)N * (double)d >= 2.0e8;
}

extern "C" size_t nw_knn_workspace_bytes(int64_t B, int64_t N, int64_t d, int64_t k) {
    return nw::knn_workspace_bytes(nw::FORM_SPLIT, B, N, d, k);
}

extern "C" size_t nw_knn_f16_workspace_bytes(int64_t B, int64_t N, int64_t d, int64_t k) {
    return nw::knn_workspace_bytes(nw::FORM_HALF, B, N, d, k);
}

// The argument rules of every neighbour-search entry, then the launch (B == 0 answers NW_OK there, after the shape rules)
static int knn_checked(const nw::KnnCall& c) {
    if (c.B < 0 || c.N < 0 || c.d < 0) return NW_ERR_INVALID_ARG;
    if (bad_kind(c.kind)) return NW_ERR_UNSUPPORTED;
    if (c.B > 0 && (!c.q || !c.s_rows || !c.s_scale || !c.s_norm2 || !c.idx)) return NW_ERR_INVALID_ARG;
    if (c.kind == NW_SCORE_CLIP && !c.logit_scale_dev) return NW_ERR_INVALID_ARG;
    if ((reinterpret_cast<uintptr_t>(c.s_rows) | reinterpret_cast<uintptr_t>(c.q) | reinterpret_cast<uintptr_t>(c.workspace)) & 15)
        return NW_ERR_INVALID_ARG;
    return nw::launch_knn(c);
}

extern "C" int nw_knn_f32(const float* q, const float* s_split, const float* s_scale, const float* s_norm2, int64_t* idx_out,
                          float* val_out, void* workspace, size_t workspace_bytes, int64_t B, int64_t N, int64_t d,
                          int64_t k, int kind, const float* logit_scale_dev, void* stream) {
    return knn_checked({q, s_split, s_scale, s_norm2, idx_out, val_out, workspace, workspace_bytes, B, N, d, k, kind,
                        logit_scale_dev, static_cast<hipStream_t>(stream), nw::FORM_SPLIT, nullptr, nullptr, 0});
}

extern "C" int nw_knn_window_f32(const float* q, const float* s_split, const float* s_scale, const float* s_norm2,
                                 const int32_t* row_lo, const int32_t* row_hi, int exclude, int64_t* idx_out, float* val_out,
                                 void* workspace, size_t workspace_bytes, int64_t B, int64_t N, int64_t d, int64_t k, int kind,
                                 const float* logit_scale_dev, void* stream) {
    if (!row_lo || !row_hi) return NW_ERR_INVALID_ARG;   // (the search without a window is nw_knn_f32)
    return knn_checked({q, s_split, s_scale, s_norm2, idx_out, val_out, workspace, workspace_bytes, B, N, d, k, kind,
                        logit_scale_dev, static_cast<hipStream_t>(stream), nw::FORM_SPLIT, row_lo, row_hi, exclude});
}

extern "C" int nw_knn_f16(const float* q, const void* s_f16, const float* s_scale, const float* s_norm2, int64_t* idx_out,
                          float* val_out, void* workspace, size_t workspace_bytes, int64_t B, int64_t N, int64_t d, int64_t k,
                          int kind, const float* logit_scale_dev, const nw_fwd_opts* opts, void* stream) {
    OptsGuard opts_guard(opts);   // (persistent_wgs is read; a struct too short to hold it counts as no options)
    return knn_checked({q, s_f16, s_scale, s_norm2, idx_out, val_out, workspace, workspace_bytes, B, N, d, k, kind,
                        logit_scale_dev, static_cast<hipStream_t>(stream), nw::FORM_HALF, nullptr, nullptr, 0});
}

extern "C" int nw_knn_merge_f32(const float* vals, const int32_t* rows, const int32_t* labels, int64_t G, int64_t B, int64_t kc,
                                int64_t stride_g, int64_t k, int64_t C, int64_t* idx_out, float* val_out, int64_t* label_out,
                                float* out, void* stream) {
    if (G < 0 || B < 0 || kc < 0 || stride_g < 0 || k < 0 || C < 0) return NW_ERR_INVALID_ARG;
    if (!vals || !rows || !labels || !idx_out) return NW_ERR_INVALID_ARG;
    if (G > 1 && stride_g < B * kc) return NW_ERR_INVALID_ARG;   // shards that overlap
    return nw::launch_knn_merge(vals, rows, labels, G, B, kc, stride_g, k, C, idx_out, val_out, label_out, out,
                                static_cast<hipStream_t>(stream));
}

extern "C" int nw_debug_tile_timing(int enable) { return nw::tile_timer_enable(enable != 0); }

extern "C" int nw_debug_tile_timing_read(double* total_us, int64_t* launches) {
    return nw::tile_timer_read(total_us, launches);
}

extern "C" int nw_fwd_influence_f32(const float* q, const float* s, const int64_t* sy, const float* s_norm2,
                                    const float* s_split, const float* s_scale, const int64_t* qy, float* out,
                                    float* lse_out, float* infl_out, void* workspace, size_t workspace_bytes,
                                    int64_t B, int64_t N, int64_t d, int64_t C, int kind,
                                    const float* logit_scale_dev, const nw_fwd_opts* opts, void* stream) {
    OptsGuard opts_guard(opts);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (B < 0 || N < 0 || d < 0 || C < 0) return NW_ERR_INVALID_ARG;
    if (nw::fwd_opts().operand_form != 0) return NW_ERR_UNSUPPORTED;   // influences need the score matrix: split or fp32 operands
    if (B == 0) return NW_OK;
    if (N == 0 || C == 0)   // no supports: log(0 + 1e-12) and nothing to score
        return nw_fwd_f32(q, s, sy, s_norm2, s_split, s_scale, out, nullptr, lse_out, nullptr, workspace, workspace_bytes,
                          B, N, d, C, kind, logit_scale_dev, 0, 0, opts, stream);
    if (!qy || !infl_out || !out) return NW_ERR_INVALID_ARG;
    const nw::FwdLayout L = nw::fwd_layout(B, N, d, C, workspace);
    if (!L.fits(workspace_bytes)) return NW_ERR_WORKSPACE;
    float* lse = lse_out ? lse_out : L.at(L.lse);
    // scores into infl_out (fused tile kernel when eligible, else the score kernel of the two-kernel path)
    const int rc = fwd_f32(q, s, sy, s_norm2, s_split, s_scale, out, infl_out, lse, nullptr, workspace, workspace_bytes, &L,
                           B, N, d, C, kind, logit_scale_dev, 0, 0, st);
    if (rc != NW_OK) return rc;
    return nw::launch_influence(out, qy, infl_out, sy, lse, infl_out, B, N, C, st);
}

extern "C" int nw_aggregate_f32(const float* scores, const int64_t* sy, float* out, float* lse_out, float* weights_out,
                                int64_t B, int64_t N, int64_t C, int labels_batched, void* stream) {
    if (B < 0 || N < 0 || C < 0) return NW_ERR_INVALID_ARG;
    if (B == 0) return NW_OK;
    if ((!out && C > 0) || (N > 0 && (!scores || !sy))) return NW_ERR_INVALID_ARG;
    return nw::launch_aggregate(scores, sy, labels_batched, out, lse_out, weights_out, nullptr, nullptr, nullptr, B, N, C,
                                static_cast<hipStream_t>(stream));
}
