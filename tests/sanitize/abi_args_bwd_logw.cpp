// Host-only exercise of nw_bwd_query_logw_f32 and nw_bwd_logw_workspace_bytes (include/nwhead_hip.h) under AddressSanitizer +
// UndefinedBehaviorSanitizer, like abi_args_fwd_weighted.cpp: built by `make -C nwhead_amd/csrc sanitize_bwd_logw` from the
// library's own sources with --cuda-host-only against hip_stubs.cpp.  Every call here must be refused BEFORE anything is
// launched (or, with B == 0, answered without touching anything), with the documented status and without a sanitizer
// report.
#include <cstdint>
#include <cstdio>
#include <vector>
#include "../../include/nwhead_hip.h"
#include "expect.h"

int main() {
    alignas(16) static float F[4096];
    alignas(16) static char ws[256];
    std::vector<int64_t> lab(64, 0);
    std::vector<int32_t> win(64, 0);
    const int64_t* SY = lab.data();
    const int32_t *LO = win.data(), *HI = win.data() + 32;
    const int E = NW_SCORE_EUCLIDEAN;

    // ================================ nw_bwd_logw_workspace_bytes
    const size_t need_ga = nw_bwd_logw_workspace_bytes(8, 1000, 64, 5, 0, 0);
    const size_t need_both = nw_bwd_logw_workspace_bytes(8, 1000, 64, 5, 0, 1);
    EXPECT(need_ga > 0, 1);
    EXPECT(need_both > need_ga, 1);
    EXPECT(need_both > nw_bwd_query_workspace_bytes(8, 1000, 64, 5, 0), 1);
    EXPECT(need_both - nw_bwd_query_workspace_bytes(8, 1000, 64, 5, 0) <= (size_t)64 * 16 * 4 + 256, 1);   // 1 query tile x 16 row tiles
    for (int gq = 0; gq < 2; ++gq) {
        EXPECT(nw_bwd_logw_workspace_bytes(0, 1000, 64, 5, 0, gq), 0);
        EXPECT(nw_bwd_logw_workspace_bytes(-1, 1000, 64, 5, 0, gq), 0);
        EXPECT(nw_bwd_logw_workspace_bytes(8, -1, 64, 5, 0, gq), 0);
        EXPECT(nw_bwd_logw_workspace_bytes(8, 25, 64, 5, 0, gq), 0);
        EXPECT(nw_bwd_logw_workspace_bytes(8, 1000, 100, 5, 0, gq), 0);
        EXPECT(nw_bwd_logw_workspace_bytes(8, 1000, 64, 0, 0, gq), 0);
        EXPECT(nw_bwd_logw_workspace_bytes(8, 1000, 64, 5, 1 << 30, gq) > 0, 1);   // chunks are clamped to the tiles
    }

    // ================================ nw_bwd_query_logw_f32
#define BWD(q, s, sy, a, lo, hi, ex, lse, out, gout, gq, ga, wsp, wsb, B, N, d, C, kind, chunks) \
    nw_bwd_query_logw_f32(q, s, F, F, sy, a, lo, hi, ex, lse, out, gout, gq, ga, nullptr, wsp, wsb, B, N, d, C, kind, nullptr, chunks, nullptr)
    for (int with_gq = 0; with_gq < 2; ++with_gq) {
        float* GQ = with_gq ? F : nullptr;
        const size_t need = with_gq ? need_both : need_ga;
        // the weights and their gradient are required; the window is both arrays or neither
        EXPECT(BWD(F, F, SY, nullptr, LO, HI, 0, F, F, F, GQ, F, ws, sizeof ws, 8, 1000, 64, 5, E, 0), NW_ERR_INVALID_ARG);
        EXPECT(BWD(F, F, SY, F, LO, HI, 0, F, F, F, GQ, nullptr, ws, sizeof ws, 8, 1000, 64, 5, E, 0), NW_ERR_INVALID_ARG);
        EXPECT(BWD(F, F, SY, F, LO, nullptr, 0, F, F, F, GQ, F, ws, sizeof ws, 8, 1000, 64, 5, E, 0), NW_ERR_INVALID_ARG);
        EXPECT(BWD(F, F, SY, F, nullptr, HI, 1, F, F, F, GQ, F, ws, sizeof ws, 8, 1000, 64, 5, E, 0), NW_ERR_INVALID_ARG);
        for (int windowed = 0; windowed < 2; ++windowed) {
            const int32_t *lo = windowed ? LO : nullptr, *hi = windowed ? HI : nullptr;
            for (int ex = 0; ex < 2; ++ex) {
                EXPECT(BWD(F, F, SY, F, lo, hi, ex, F, F, F, GQ, F, ws, sizeof ws, -1, 1000, 64, 5, E, 0), NW_ERR_INVALID_ARG);
                EXPECT(BWD(F, F, SY, F, lo, hi, ex, F, F, F, GQ, F, ws, sizeof ws, 8, 1000, 64, 5, E, -1), NW_ERR_INVALID_ARG);
                EXPECT(BWD(nullptr, F, SY, F, lo, hi, ex, F, F, F, GQ, F, ws, sizeof ws, 8, 1000, 64, 5, E, 0), NW_ERR_INVALID_ARG);
                EXPECT(BWD(F, nullptr, SY, F, lo, hi, ex, F, F, F, GQ, F, ws, sizeof ws, 8, 1000, 64, 5, E, 0), NW_ERR_INVALID_ARG);
                EXPECT(BWD(F, F, nullptr, F, lo, hi, ex, F, F, F, GQ, F, ws, sizeof ws, 8, 1000, 64, 5, E, 0), NW_ERR_INVALID_ARG);
                EXPECT(BWD(F, F, SY, F, lo, hi, ex, nullptr, F, F, GQ, F, ws, sizeof ws, 8, 1000, 64, 5, E, 0), NW_ERR_INVALID_ARG);
                EXPECT(BWD(F, F, SY, F, lo, hi, ex, F, nullptr, F, GQ, F, ws, sizeof ws, 8, 1000, 64, 5, E, 0), NW_ERR_INVALID_ARG);
                EXPECT(BWD(F, F, SY, F, lo, hi, ex, F, F, nullptr, GQ, F, ws, sizeof ws, 8, 1000, 64, 5, E, 0), NW_ERR_INVALID_ARG);
                EXPECT(BWD(F, F, SY, F, lo, hi, ex, F, F, F, GQ, F, ws, sizeof ws, 8, 1000, 64, 5, NW_SCORE_CLIP, 0), NW_ERR_INVALID_ARG);
                // outside the regime of nw_bwd_query_weighted_f32
                EXPECT(BWD(F, F, SY, F, lo, hi, ex, F, F, F, GQ, F, ws, sizeof ws, 8, 1000, 64, 5, 99, 0), NW_ERR_UNSUPPORTED);
                EXPECT(BWD(F, F, SY, F, lo, hi, ex, F, F, F, GQ, F, ws, sizeof ws, 8, 1000, 100, 5, E, 0), NW_ERR_UNSUPPORTED);
                EXPECT(BWD(F, F, SY, F, lo, hi, ex, F, F, F, GQ, F, ws, sizeof ws, 8, 1000, 16, 5, E, 0), NW_ERR_UNSUPPORTED);
                EXPECT(BWD(F, F, SY, F, lo, hi, ex, F, F, F, GQ, F, ws, sizeof ws, 8, 25, 64, 5, E, 0), NW_ERR_UNSUPPORTED);
                EXPECT(BWD(F, F, SY, F, lo, hi, ex, F, F, F, GQ, F, ws, sizeof ws, 8, 1000, 64, 0, E, 0), NW_ERR_UNSUPPORTED);
                EXPECT(BWD(F + 1, F, SY, F, lo, hi, ex, F, F, F, GQ, F, ws, sizeof ws, 8, 1000, 64, 5, E, 0), NW_ERR_UNSUPPORTED);
                EXPECT(BWD(F, F + 1, SY, F, lo, hi, ex, F, F, F, GQ, F, ws, sizeof ws, 8, 1000, 64, 5, E, 0), NW_ERR_UNSUPPORTED);
                EXPECT(BWD(F, F, SY, F + 1, lo, hi, ex, F, F, F, GQ, F, ws, sizeof ws, 8, 1000, 64, 5, E, 0), NW_ERR_UNSUPPORTED);
                EXPECT(BWD(F, F, SY, F, lo, hi, ex, F, F, F, GQ, F + 1, ws, sizeof ws, 8, 1000, 64, 5, E, 0), NW_ERR_UNSUPPORTED);   // glogw's alignment
                if (with_gq) EXPECT(BWD(F, F, SY, F, lo, hi, ex, F, F, F, F + 1, F, ws, sizeof ws, 8, 1000, 64, 5, E, 0), NW_ERR_UNSUPPORTED);
                // the workspace: the size of the variant that is called
                EXPECT(BWD(F, F, SY, F, lo, hi, ex, F, F, F, GQ, F, ws, sizeof ws, 8, 1000, 64, 5, E, 0), NW_ERR_WORKSPACE);
                EXPECT(BWD(F, F, SY, F, lo, hi, ex, F, F, F, GQ, F, nullptr, need, 8, 1000, 64, 5, E, 0), NW_ERR_WORKSPACE);
                EXPECT(BWD(F, F, SY, F, lo, hi, ex, F, F, F, GQ, F, ws, need - 1, 8, 1000, 64, 5, E, 0), NW_ERR_WORKSPACE);
                EXPECT(BWD(F, F, SY, F, lo, hi, ex, F, F, F, GQ, F, ws + 4, need, 8, 1000, 64, 5, E, 0), NW_ERR_UNSUPPORTED);
                // B == 0: NW_OK, nothing is read, nothing is written (glogw included), nothing is launched
                EXPECT(BWD(nullptr, nullptr, nullptr, nullptr, lo, hi, ex, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, 1000, 64, 5, E, 0), NW_OK);
                F[0] = 42.f;
                EXPECT(BWD(F, F, SY, F, lo, hi, ex, F, F, F, GQ, F, ws, sizeof ws, 0, 1000, 64, 5, E, 0), NW_OK);
                EXPECT(F[0] == 42.f, 1);
            }
        }
    }
    std::printf(failures ? "abi_args_bwd_logw: %d FAILED\n" : "abi_args_bwd_logw: all argument checks refused as documented\n", failures);
    return failures ? 1 : 0;
}
