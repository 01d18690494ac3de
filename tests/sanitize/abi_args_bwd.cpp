// Host-only exercise of the head's backward entries (include/nwhead_hip.h: nw_bwd_f32, nw_bwd_bank_f32,
// nw_aggregate_bwd_f32, nw_bwd_workspace_bytes, nw_bwd_uses_split, nw_debug_bwd_plan) under AddressSanitizer +
// UndefinedBehaviorSanitizer, like abi_args_bwd_query.cpp: built by `make -C nwhead_amd/csrc sanitize_bwd` from the
// library's own sources with --cuda-host-only against hip_stubs.cpp.  Every call here must be refused BEFORE anything is
// launched (or, for an empty shape, answered), with the documented status, in the documented precedence, and without a
// sanitizer report.  The workspace is never touched on the host: a small buffer stands in for any claimed size.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../include/nwhead_hip.h"
#include "expect.h"

static const int E = NW_SCORE_EUCLIDEAN;
alignas(16) static float F[4096];
alignas(16) static char ws[256];
static int64_t SY[64];

// nw_bwd_bank_f32 with every operand in order; the arguments a case is about are passed explicitly
static int bank(const float* q, const float* s, const float* n2, const float* split, const float* scale, void* wsp, size_t wsb,
                int64_t B, int64_t N, int64_t d, int64_t C, int kind = E, const float* ls = nullptr, int sup = 0, float* gq = F,
                float* gs = F) {
    return nw_bwd_bank_f32(q, s, n2, split, scale, SY, F, F, F, F, gq, gs, nullptr, wsp, wsb, B, N, d, C, kind, ls, sup, 0, nullptr);
}

// the plan of one shape against the two older questions about it; returns the route
static int plan_agrees(int64_t B, int64_t N, int64_t d, int64_t C, int sup) {
    nw_bwd_plan p;
    std::memset(&p, 0xFF, sizeof p);
    EXPECT(nw_debug_bwd_plan(B, N, d, C, sup, &p), NW_OK);
    EXPECT(p.total, nw_bwd_workspace_bytes(B, N, d, C, E, sup));
    EXPECT(p.route == 2, nw_bwd_uses_split(B, N, d, C, sup));
    EXPECT(p.off[0], 0);
    for (int i = 1; i < NW_BWD_AREAS - 1; ++i) EXPECT(p.off[i], p.off[i - 1] + p.bytes[i - 1]);
    EXPECT(p.off[NW_BWD_AREAS - 1] + p.bytes[NW_BWD_AREAS - 1], p.total);
    return p.route;
}

int main() {
    // ---- the three host questions over the edge shapes, under every knob state
    const int64_t shapes[][4] = {{16, 38300, 32, 16}, {16, 38305, 32, 16}, {64, 1000, 512, 37500}, {16, 256, 1024, 5}, {15, 280, 1024, 5},
                                 {16, 255, 1056, 5},  {16, 256, 992, 5},   {16, 300, 1022, 5},     {2, 30, 8, 40880},  {2, 30, 8, 40881},
                                 {1, 0, 64, 5},       {1, 1, 0, 0},        {256, 10000, 512, 200}, {3, 3000, 36, 7},   {64, 1024, 64, 5}};
    const int unset = -2147483647 - 1, split_knob[] = {unset, 0, 1}, no_mfma[] = {unset, 1};
    for (int sk : split_knob)
        for (int nm : no_mfma) {
            EXPECT(nw_debug_set("bwd_split", sk), NW_OK);
            EXPECT(nw_debug_set("bwd_no_mfma", nm), NW_OK);
            for (const auto& sh : shapes)
                for (int sup = 0; sup < 2; ++sup) {
                    const int route = plan_agrees(sh[0], sh[1], sh[2], sh[3], sup);
                    if (nm == 1 || sup) EXPECT(route, 0);
                    if (sk == 0) EXPECT(route == 2, 0);
                }
        }
    EXPECT(nw_debug_set("bwd_split", unset), NW_OK);
    EXPECT(nw_debug_set("bwd_no_mfma", unset), NW_OK);
    EXPECT(plan_agrees(16, 38300, 32, 16, 0), 2);
    EXPECT(plan_agrees(16, 38305, 32, 16, 0), 1);
    EXPECT(plan_agrees(16, 256, 992, 5, 0), 0);
    {
        nw_bwd_plan p, zero;
        std::memset(&zero, 0, sizeof zero);
        EXPECT(nw_debug_bwd_plan(64, 1024, 64, 5, 0, nullptr), NW_ERR_INVALID_ARG);
        EXPECT(nw_debug_bwd_plan(-1, 1024, 64, 5, 0, &p), NW_ERR_INVALID_ARG);
        EXPECT(nw_debug_bwd_plan(64, -1, 64, 5, 0, &p), NW_ERR_INVALID_ARG);
        EXPECT(nw_debug_bwd_plan(64, 1024, -64, 5, 0, &p), NW_ERR_INVALID_ARG);
        EXPECT(nw_debug_bwd_plan(64, 1024, 64, -5, 0, &p), NW_ERR_INVALID_ARG);
        std::memset(&p, 0xFF, sizeof p);
        EXPECT(nw_debug_bwd_plan(0, 1024, 64, 5, 0, &p), NW_OK);
        EXPECT(std::memcmp(&p, &zero, sizeof p), 0);
        EXPECT(nw_debug_bwd_plan(2, 30, 8, 40880, 0, &p), NW_OK);
        EXPECT(p.status, NW_OK);
        EXPECT(p.coeff_lds_bytes, 160 * 1024);
        EXPECT(nw_debug_bwd_plan(2, 30, 8, 40881, 0, &p), NW_OK);
        EXPECT(p.status, NW_ERR_UNSUPPORTED);
    }
    EXPECT(nw_bwd_workspace_bytes(0, 1000, 64, 5, E, 0), 0);
    EXPECT(nw_bwd_workspace_bytes(-1, 1000, 64, 5, E, 0), 0);
    EXPECT(nw_bwd_workspace_bytes(16, -1, 64, 5, E, 0), 0);
    EXPECT(nw_bwd_workspace_bytes(1, 0, 64, 5, E, 0), 3 * 256);        // A, Rs and sn2 empty; rq, gls, qn2 one float each
    EXPECT(nw_bwd_workspace_bytes(1, 0, 64, 5, E, 0) == nw_bwd_workspace_bytes(1, 0, -64, -5, 99, 0), 1);
    EXPECT(nw_bwd_uses_split(16, 0, 64, 5, 0), 0);
    EXPECT(nw_bwd_uses_split(16, 1000, 0, 5, 0), 0);
    EXPECT(nw_bwd_uses_split(16, 1000, 64, -1, 0), 0);
    EXPECT(nw_bwd_uses_split(0, 1000, 64, 5, 0), 0);

    // ---- nw_bwd_bank_f32 / nw_bwd_f32: every refusal that returns before a launch.  (2, 30, 8, 5) runs on the VALU route,
    // (64, 1024, 64, 5) on the split route, and on the fp32 matrix cores with bwd_split = 0
    const size_t small = nw_bwd_workspace_bytes(2, 30, 8, 5, E, 0), big = nw_bwd_workspace_bytes(64, 1024, 64, 5, E, 0);
    EXPECT(small > 0 && small <= big, 1);
    // a bank given in part, before anything else is looked at
    EXPECT(bank(F, F, F, F, nullptr, ws, big, 64, 1024, 64, 5), NW_ERR_INVALID_ARG);
    EXPECT(bank(F, F, F, nullptr, F, ws, big, 64, 1024, 64, 5), NW_ERR_INVALID_ARG);
    EXPECT(bank(F, F, nullptr, F, F, ws, big, 64, 1024, 64, 5), NW_ERR_INVALID_ARG);
    EXPECT(bank(F, F, F, F, nullptr, ws, big, 64, 1024, 64, 5, 99), NW_ERR_INVALID_ARG);      // ... not the kind
    EXPECT(bank(F, F, F, F, nullptr, ws, big, 0, 1024, 64, 5), NW_ERR_INVALID_ARG);           // ... not an empty batch
    // a whole bank that cannot be one: per-query supports, rows that are no split rows, a misaligned image
    EXPECT(bank(F, F, F, F, F, ws, big, 64, 1024, 64, 5, E, nullptr, 1), NW_ERR_INVALID_ARG);
    EXPECT(bank(F, F, F, F, F, ws, big, 64, 1024, 48, 5), NW_ERR_INVALID_ARG);
    EXPECT(bank(F, F, F, F + 1, F, ws, big, 64, 1024, 64, 5), NW_ERR_INVALID_ARG);
    EXPECT(bank(F, F, F, F + 1, F, ws, big, 64, 1024, 64, 5, 99), NW_ERR_INVALID_ARG);        // ... before the kind
    // negative sizes
    EXPECT(bank(F, F, nullptr, nullptr, nullptr, ws, small, -2, 30, 8, 5), NW_ERR_INVALID_ARG);
    EXPECT(bank(F, F, nullptr, nullptr, nullptr, ws, small, 2, -30, 8, 5), NW_ERR_INVALID_ARG);
    EXPECT(bank(F, F, nullptr, nullptr, nullptr, ws, small, 2, 30, -8, 5), NW_ERR_INVALID_ARG);
    EXPECT(bank(F, F, nullptr, nullptr, nullptr, ws, small, 2, 30, 8, -5), NW_ERR_INVALID_ARG);
    EXPECT(bank(F, F, nullptr, nullptr, nullptr, ws, small, -2, 30, 8, 5, 99), NW_ERR_INVALID_ARG);   // ... before the kind
    // a bad kind, CLIP without its scale
    EXPECT(bank(F, F, nullptr, nullptr, nullptr, ws, small, 2, 30, 8, 5, 99), NW_ERR_UNSUPPORTED);
    EXPECT(bank(F, F, nullptr, nullptr, nullptr, ws, small, 2, 30, 8, 5, -1), NW_ERR_UNSUPPORTED);
    EXPECT(bank(nullptr, F, nullptr, nullptr, nullptr, ws, small, 2, 30, 8, 5, 99), NW_ERR_UNSUPPORTED);   // ... before the operands
    EXPECT(bank(F, F, nullptr, nullptr, nullptr, ws, small, 2, 30, 8, 5, NW_SCORE_CLIP, nullptr), NW_ERR_INVALID_ARG);
    EXPECT(bank(F, F, nullptr, nullptr, nullptr, ws, small, 0, 30, 8, 5, NW_SCORE_CLIP, nullptr), NW_ERR_INVALID_ARG);   // ... even when empty
    // an empty shape with nothing to clear: NW_OK, nothing read, nothing launched
    EXPECT(nw_bwd_bank_f32(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                           nullptr, nullptr, 0, 0, 30, 8, 5, E, nullptr, 0, 0, nullptr), NW_OK);
    EXPECT(nw_bwd_f32(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, 0, 0, 0, E,
                      nullptr, 1, 1, nullptr), NW_OK);
    // null operands, one at a time
    {
        const void* a[9] = {F, F, SY, F, F, F, F, F, F};   // q, s, sy, scores, lse, out, gout, gq, gs
        for (int i = 0; i < 9; ++i) {
            const void* b[9];
            for (int k = 0; k < 9; ++k) b[k] = k == i ? nullptr : a[k];
            EXPECT(nw_bwd_f32((const float*)b[0], (const float*)b[1], (const int64_t*)b[2], (const float*)b[3], (const float*)b[4],
                              (const float*)b[5], (const float*)b[6], (float*)b[7], (float*)b[8], nullptr, ws, small, 2, 30, 8, 5, E,
                              nullptr, 0, 0, nullptr), NW_ERR_INVALID_ARG);
        }
        EXPECT(bank(nullptr, F, nullptr, nullptr, nullptr, nullptr, 0, 2, 30, 8, 5), NW_ERR_INVALID_ARG);   // ... before the workspace
    }
    // sizes past the launch grids
    EXPECT(bank(F, F, nullptr, nullptr, nullptr, ws, small, (int64_t)1 << 31, 1, 8, 5), NW_ERR_INVALID_ARG);
    EXPECT(bank(F, F, nullptr, nullptr, nullptr, ws, small, 2, (int64_t)1 << 31, 8, 5), NW_ERR_INVALID_ARG);
    EXPECT(bank(F, F, nullptr, nullptr, nullptr, ws, small, 2, 30, 65536 * 256, 5), NW_ERR_INVALID_ARG);
    // the workspace: short, null
    EXPECT(bank(F, F, nullptr, nullptr, nullptr, ws, small - 1, 2, 30, 8, 5), NW_ERR_WORKSPACE);
    EXPECT(bank(F, F, nullptr, nullptr, nullptr, nullptr, small, 2, 30, 8, 5), NW_ERR_WORKSPACE);
    EXPECT(bank(F, F, nullptr, nullptr, nullptr, ws, 0, 2, 30, 8, 5), NW_ERR_WORKSPACE);
    EXPECT(bank(F, F, F, F, F, ws, big - 1, 64, 1024, 64, 5), NW_ERR_WORKSPACE);
    EXPECT(bank(F + 1, F, nullptr, nullptr, nullptr, ws, big - 1, 64, 1024, 64, 5), NW_ERR_WORKSPACE);   // ... before the alignment
    EXPECT(bank(F, F, nullptr, nullptr, nullptr, ws, small - 1, 2, 30, 8, 40881), NW_ERR_WORKSPACE);      // ... before the class limit
    // the class limit of the launcher: 80 + C floats of LDS past 160 KiB
    EXPECT(nw_bwd_workspace_bytes(2, 30, 8, 40881, E, 0), small);       // the class count is no part of any buffer
    EXPECT(bank(F, F, nullptr, nullptr, nullptr, ws, small, 2, 30, 8, 40881), NW_ERR_UNSUPPORTED);
    EXPECT(nw_bwd_f32(F, F, SY, F, F, F, F, F, F, nullptr, ws, small, 2, 30, 8, 40881, E, nullptr, 0, 0, nullptr), NW_ERR_UNSUPPORTED);
    {   // ... on a matrix-core route, where it comes before the alignment
        const size_t need = nw_bwd_workspace_bytes(64, 1000, 512, 41000, E, 0);
        EXPECT(nw_bwd_uses_split(64, 1000, 512, 41000, 0), 0);
        EXPECT(bank(F + 1, F, nullptr, nullptr, nullptr, ws, need, 64, 1000, 512, 41000), NW_ERR_UNSUPPORTED);
    }
    // misaligned operands on the two matrix-core routes (the VALU route takes any alignment: it would launch)
    for (int sk : {unset, 0}) {
        EXPECT(nw_debug_set("bwd_split", sk), NW_OK);
        const size_t need = nw_bwd_workspace_bytes(64, 1024, 64, 5, E, 0);
        EXPECT(nw_bwd_uses_split(64, 1024, 64, 5, 0), sk == unset);
        EXPECT(need > small, 1);
        EXPECT(bank(F + 1, F, nullptr, nullptr, nullptr, ws, need, 64, 1024, 64, 5), NW_ERR_INVALID_ARG);
        EXPECT(bank(F, F + 1, nullptr, nullptr, nullptr, ws, need, 64, 1024, 64, 5), NW_ERR_INVALID_ARG);
        EXPECT(bank(F, F, nullptr, nullptr, nullptr, ws, need, 64, 1024, 64, 5, E, nullptr, 0, F + 1, F), NW_ERR_INVALID_ARG);
        EXPECT(bank(F, F, nullptr, nullptr, nullptr, ws, need, 64, 1024, 64, 5, E, nullptr, 0, F, F + 1), NW_ERR_INVALID_ARG);
        EXPECT(bank(F, F + 1, F, F, F, ws, need, 64, 1024, 64, 5), NW_ERR_INVALID_ARG);
    }
    EXPECT(nw_debug_set("bwd_split", unset), NW_OK);

    // ---- nw_aggregate_bwd_f32
    EXPECT(nw_aggregate_bwd_f32(F, SY, F, F, F, F, -1, 30, 5, 0, nullptr), NW_ERR_INVALID_ARG);
    EXPECT(nw_aggregate_bwd_f32(F, SY, F, F, F, F, 2, -30, 5, 0, nullptr), NW_ERR_INVALID_ARG);
    EXPECT(nw_aggregate_bwd_f32(F, SY, F, F, F, F, 2, 30, -5, 0, nullptr), NW_ERR_INVALID_ARG);
    EXPECT(nw_aggregate_bwd_f32(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 30, 5, 0, nullptr), NW_OK);
    EXPECT(nw_aggregate_bwd_f32(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 2, 0, 5, 0, nullptr), NW_OK);
    EXPECT(nw_aggregate_bwd_f32(nullptr, SY, F, F, F, F, 2, 30, 5, 0, nullptr), NW_ERR_INVALID_ARG);
    EXPECT(nw_aggregate_bwd_f32(F, nullptr, F, F, F, F, 2, 30, 5, 0, nullptr), NW_ERR_INVALID_ARG);
    EXPECT(nw_aggregate_bwd_f32(F, SY, nullptr, F, F, F, 2, 30, 5, 0, nullptr), NW_ERR_INVALID_ARG);
    EXPECT(nw_aggregate_bwd_f32(F, SY, F, nullptr, F, F, 2, 30, 5, 0, nullptr), NW_ERR_INVALID_ARG);
    EXPECT(nw_aggregate_bwd_f32(F, SY, F, F, nullptr, F, 2, 30, 5, 0, nullptr), NW_ERR_INVALID_ARG);
    EXPECT(nw_aggregate_bwd_f32(F, SY, F, F, F, nullptr, 2, 30, 5, 0, nullptr), NW_ERR_INVALID_ARG);
    EXPECT(nw_aggregate_bwd_f32(F, SY, F, F, F, F, (int64_t)1 << 31, 30, 5, 0, nullptr), NW_ERR_INVALID_ARG);
    EXPECT(nw_aggregate_bwd_f32(F, SY, F, F, F, F, 2, 30, 40881, 0, nullptr), NW_ERR_UNSUPPORTED);
    EXPECT(nw_aggregate_bwd_f32(F, SY, F, F, F, F, 2, 3000, 40881, 1, nullptr), NW_ERR_UNSUPPORTED);

    std::printf(failures ? "abi_args_bwd: %d FAILED\n" : "abi_args_bwd: all argument checks refused as documented\n", failures);
    return failures ? 1 : 0;
}
