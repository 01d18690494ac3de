// Host-only exercise of nw_bwd_query_f32 / nw_bwd_query_workspace_bytes (include/nwhead_hip.h) under AddressSanitizer +
// UndefinedBehaviorSanitizer, like abi_args_fwd_window.cpp: built by `make -C nwhead_amd/csrc sanitize_bwd_query` from the
// library's own sources with --cuda-host-only against hip_stubs.cpp.  Every call here must be refused BEFORE anything is
// launched (or, with B == 0, answered), with the documented status and without a sanitizer report.
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
    const int E = NW_SCORE_EUCLIDEAN;
    // ---- the workspace: none outside the regime, more for more chunks, clamped at the tile count
    const size_t need = nw_bwd_query_workspace_bytes(8, 1000, 64, 5, 0);
    EXPECT(need > sizeof ws, 1);
    EXPECT(nw_bwd_query_workspace_bytes(0, 1000, 64, 5, 0), 0);
    EXPECT(nw_bwd_query_workspace_bytes(-1, 1000, 64, 5, 0), 0);
    EXPECT(nw_bwd_query_workspace_bytes(8, 1000, 100, 5, 0), 0);
    EXPECT(nw_bwd_query_workspace_bytes(8, 1000, 16, 5, 0), 0);
    EXPECT(nw_bwd_query_workspace_bytes(8, 25, 64, 5, 0), 0);
    EXPECT(nw_bwd_query_workspace_bytes(8, 1000, 64, 0, 0), 0);
    EXPECT(nw_bwd_query_workspace_bytes(8, 1000, 64, 5, 2) > nw_bwd_query_workspace_bytes(8, 1000, 64, 5, 1), 1);
    EXPECT(nw_bwd_query_workspace_bytes(8, 1000, 64, 5, 1000) == nw_bwd_query_workspace_bytes(8, 1000, 64, 5, 1 << 30), 1);
    EXPECT(nw_bwd_query_workspace_bytes(256, 50000, 512, 200, 0) < (size_t)256 * 50000, 1);
    EXPECT(nw_bwd_query_workspace_bytes(256, 400000, 256, 200, 0) < (size_t)256 * 400000, 1);
    for (int w = 0; w < 2; ++w) {      // with a window and without
        const int32_t *LO = w ? win.data() : nullptr, *HI = w ? win.data() + 32 : nullptr;
#define CALL(q, s, sc, n2, sy, lse, out, gout, gq, wsp, wsb, B, N, d, C, kind, ls, chunks) \
    nw_bwd_query_f32(q, s, sc, n2, sy, LO, HI, w, lse, out, gout, gq, nullptr, wsp, wsb, B, N, d, C, kind, ls, chunks, nullptr)
        // negative sizes
        EXPECT(CALL(F, F, F, F, SY, F, F, F, F, ws, sizeof ws, -1, 1000, 64, 5, E, nullptr, 0), NW_ERR_INVALID_ARG);
        EXPECT(CALL(F, F, F, F, SY, F, F, F, F, ws, sizeof ws, 8, -1, 64, 5, E, nullptr, 0), NW_ERR_INVALID_ARG);
        EXPECT(CALL(F, F, F, F, SY, F, F, F, F, ws, sizeof ws, 8, 1000, -64, 5, E, nullptr, 0), NW_ERR_INVALID_ARG);
        EXPECT(CALL(F, F, F, F, SY, F, F, F, F, ws, sizeof ws, 8, 1000, 64, -5, E, nullptr, 0), NW_ERR_INVALID_ARG);
        EXPECT(CALL(F, F, F, F, SY, F, F, F, F, ws, sizeof ws, 8, 1000, 64, 5, E, nullptr, -1), NW_ERR_INVALID_ARG);
        // null operands, labels, forward results, gradients
        EXPECT(CALL(nullptr, F, F, F, SY, F, F, F, F, ws, sizeof ws, 8, 1000, 64, 5, E, nullptr, 0), NW_ERR_INVALID_ARG);
        EXPECT(CALL(F, nullptr, F, F, SY, F, F, F, F, ws, sizeof ws, 8, 1000, 64, 5, E, nullptr, 0), NW_ERR_INVALID_ARG);
        EXPECT(CALL(F, F, nullptr, F, SY, F, F, F, F, ws, sizeof ws, 8, 1000, 64, 5, E, nullptr, 0), NW_ERR_INVALID_ARG);
        EXPECT(CALL(F, F, F, nullptr, SY, F, F, F, F, ws, sizeof ws, 8, 1000, 64, 5, E, nullptr, 0), NW_ERR_INVALID_ARG);
        EXPECT(CALL(F, F, F, F, nullptr, F, F, F, F, ws, sizeof ws, 8, 1000, 64, 5, E, nullptr, 0), NW_ERR_INVALID_ARG);
        EXPECT(CALL(F, F, F, F, SY, nullptr, F, F, F, ws, sizeof ws, 8, 1000, 64, 5, E, nullptr, 0), NW_ERR_INVALID_ARG);
        EXPECT(CALL(F, F, F, F, SY, F, nullptr, F, F, ws, sizeof ws, 8, 1000, 64, 5, E, nullptr, 0), NW_ERR_INVALID_ARG);
        EXPECT(CALL(F, F, F, F, SY, F, F, nullptr, F, ws, sizeof ws, 8, 1000, 64, 5, E, nullptr, 0), NW_ERR_INVALID_ARG);
        EXPECT(CALL(F, F, F, F, SY, F, F, F, nullptr, ws, sizeof ws, 8, 1000, 64, 5, E, nullptr, 0), NW_ERR_INVALID_ARG);
        EXPECT(CALL(F, F, F, F, SY, F, F, F, F, ws, sizeof ws, 8, 1000, 64, 5, NW_SCORE_CLIP, nullptr, 0), NW_ERR_INVALID_ARG);
        // outside the regime of nw_fwd_window_f32
        EXPECT(CALL(F, F, F, F, SY, F, F, F, F, ws, sizeof ws, 8, 1000, 64, 5, 99, nullptr, 0), NW_ERR_UNSUPPORTED);
        EXPECT(CALL(F, F, F, F, SY, F, F, F, F, ws, sizeof ws, 8, 1000, 100, 5, E, nullptr, 0), NW_ERR_UNSUPPORTED);
        EXPECT(CALL(F, F, F, F, SY, F, F, F, F, ws, sizeof ws, 8, 1000, 16, 5, E, nullptr, 0), NW_ERR_UNSUPPORTED);
        EXPECT(CALL(F, F, F, F, SY, F, F, F, F, ws, sizeof ws, 8, 1000, 0, 5, E, nullptr, 0), NW_ERR_UNSUPPORTED);
        EXPECT(CALL(F, F, F, F, SY, F, F, F, F, ws, sizeof ws, 8, 25, 64, 5, E, nullptr, 0), NW_ERR_UNSUPPORTED);
        EXPECT(CALL(F, F, F, F, SY, F, F, F, F, ws, sizeof ws, 8, 0, 64, 5, E, nullptr, 0), NW_ERR_UNSUPPORTED);
        EXPECT(CALL(F, F, F, F, SY, F, F, F, F, ws, sizeof ws, 8, 1000, 64, 0, E, nullptr, 0), NW_ERR_UNSUPPORTED);
        EXPECT(CALL(F + 1, F, F, F, SY, F, F, F, F, ws, need, 8, 1000, 64, 5, E, nullptr, 0), NW_ERR_UNSUPPORTED);
        EXPECT(CALL(F, F + 1, F, F, SY, F, F, F, F, ws, need, 8, 1000, 64, 5, E, nullptr, 0), NW_ERR_UNSUPPORTED);
        EXPECT(CALL(F, F, F, F, SY, F, F, F, F + 1, ws, need, 8, 1000, 64, 5, E, nullptr, 0), NW_ERR_UNSUPPORTED);
        // the workspace
        EXPECT(CALL(F, F, F, F, SY, F, F, F, F, ws, sizeof ws, 8, 1000, 64, 5, E, nullptr, 0), NW_ERR_WORKSPACE);
        EXPECT(CALL(F, F, F, F, SY, F, F, F, F, nullptr, need, 8, 1000, 64, 5, E, nullptr, 0), NW_ERR_WORKSPACE);
        EXPECT(CALL(F, F, F, F, SY, F, F, F, F, ws, need - 1, 8, 1000, 64, 5, E, nullptr, 0), NW_ERR_WORKSPACE);
        EXPECT(CALL(F, F, F, F, SY, F, F, F, F, ws, need, 8, 1000, 64, 5, E, nullptr, 1000), NW_ERR_WORKSPACE);   // more chunks ask for more
        EXPECT(CALL(F, F, F, F, SY, F, F, F, F, ws + 4, need, 8, 1000, 64, 5, E, nullptr, 0), NW_ERR_UNSUPPORTED);
        // B == 0: NW_OK, nothing is read, nothing is launched
        EXPECT(CALL(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, 1000, 64, 5, E, nullptr, 0),
               NW_OK);
#undef CALL
    }
    // one half of a window, even with B == 0
    EXPECT(nw_bwd_query_f32(F, F, F, F, SY, win.data(), nullptr, 0, F, F, F, F, nullptr, ws, sizeof ws, 8, 1000, 64, 5, E, nullptr, 0, nullptr),
           NW_ERR_INVALID_ARG);
    EXPECT(nw_bwd_query_f32(F, F, F, F, SY, nullptr, win.data(), 1, F, F, F, F, nullptr, ws, sizeof ws, 8, 1000, 64, 5, E, nullptr, 0, nullptr),
           NW_ERR_INVALID_ARG);
    EXPECT(nw_bwd_query_f32(nullptr, nullptr, nullptr, nullptr, nullptr, win.data(), nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr,
                            nullptr, 0, 0, 1000, 64, 5, E, nullptr, 0, nullptr), NW_ERR_INVALID_ARG);
    std::printf(failures ? "abi_args_bwd_query: %d FAILED\n" : "abi_args_bwd_query: all argument checks refused as documented\n",
                failures);
    return failures ? 1 : 0;
}
