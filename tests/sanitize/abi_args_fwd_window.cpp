// Host-only exercise of nw_fwd_window_f32 (include/nwhead_hip.h) under AddressSanitizer + UndefinedBehaviorSanitizer, like
// abi_args_knn_window.cpp: built by `make -C nwhead_amd/csrc sanitize_fwd_window` from the library's own sources with
// --cuda-host-only against hip_stubs.cpp.  Every call here must be refused BEFORE anything is launched (or, with B == 0,
// answered), with the documented status and without a sanitizer report.
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
    // ---- the windowed head takes nw_fwd_f32's workspace
    const size_t need = nw_fwd_workspace_bytes(8, 1000, 64, 5);
    EXPECT(need > 0, 1);
    // ---- refused before any launch: the window itself
    EXPECT(nw_fwd_window_f32(F, F, F, F, SY, nullptr, HI, 0, F, nullptr, ws, sizeof ws, 8, 1000, 64, 5, E, nullptr, nullptr), NW_ERR_INVALID_ARG);
    EXPECT(nw_fwd_window_f32(F, F, F, F, SY, LO, nullptr, 0, F, nullptr, ws, sizeof ws, 8, 1000, 64, 5, E, nullptr, nullptr), NW_ERR_INVALID_ARG);
    EXPECT(nw_fwd_window_f32(F, F, F, F, SY, nullptr, nullptr, 1, F, nullptr, ws, sizeof ws, 8, 1000, 64, 5, E, nullptr, nullptr), NW_ERR_INVALID_ARG);
    EXPECT(nw_fwd_window_f32(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0, 0, 1000, 64, 5, E,
                             nullptr, nullptr), NW_ERR_INVALID_ARG);                                  // ... even with B == 0
    for (int ex = 0; ex < 2; ++ex) {
        // negative sizes
        EXPECT(nw_fwd_window_f32(F, F, F, F, SY, LO, HI, ex, F, nullptr, ws, sizeof ws, -1, 1000, 64, 5, E, nullptr, nullptr), NW_ERR_INVALID_ARG);
        EXPECT(nw_fwd_window_f32(F, F, F, F, SY, LO, HI, ex, F, nullptr, ws, sizeof ws, 8, -1, 64, 5, E, nullptr, nullptr), NW_ERR_INVALID_ARG);
        EXPECT(nw_fwd_window_f32(F, F, F, F, SY, LO, HI, ex, F, nullptr, ws, sizeof ws, 8, 1000, -64, 5, E, nullptr, nullptr), NW_ERR_INVALID_ARG);
        EXPECT(nw_fwd_window_f32(F, F, F, F, SY, LO, HI, ex, F, nullptr, ws, sizeof ws, 8, 1000, 64, -5, E, nullptr, nullptr), NW_ERR_INVALID_ARG);
        // null operands, labels, output
        EXPECT(nw_fwd_window_f32(nullptr, F, F, F, SY, LO, HI, ex, F, nullptr, ws, sizeof ws, 8, 1000, 64, 5, E, nullptr, nullptr), NW_ERR_INVALID_ARG);
        EXPECT(nw_fwd_window_f32(F, nullptr, F, F, SY, LO, HI, ex, F, nullptr, ws, sizeof ws, 8, 1000, 64, 5, E, nullptr, nullptr), NW_ERR_INVALID_ARG);
        EXPECT(nw_fwd_window_f32(F, F, nullptr, F, SY, LO, HI, ex, F, nullptr, ws, sizeof ws, 8, 1000, 64, 5, E, nullptr, nullptr), NW_ERR_INVALID_ARG);
        EXPECT(nw_fwd_window_f32(F, F, F, nullptr, SY, LO, HI, ex, F, nullptr, ws, sizeof ws, 8, 1000, 64, 5, E, nullptr, nullptr), NW_ERR_INVALID_ARG);
        EXPECT(nw_fwd_window_f32(F, F, F, F, nullptr, LO, HI, ex, F, nullptr, ws, sizeof ws, 8, 1000, 64, 5, E, nullptr, nullptr), NW_ERR_INVALID_ARG);
        EXPECT(nw_fwd_window_f32(F, F, F, F, SY, LO, HI, ex, nullptr, nullptr, ws, sizeof ws, 8, 1000, 64, 5, E, nullptr, nullptr), NW_ERR_INVALID_ARG);
        EXPECT(nw_fwd_window_f32(F, F, F, F, SY, LO, HI, ex, F, nullptr, ws, sizeof ws, 8, 1000, 64, 5, NW_SCORE_CLIP, nullptr, nullptr),
               NW_ERR_INVALID_ARG);                                                                   // clip without logit_scale
        // outside the regime of nw_knn_window_f32
        EXPECT(nw_fwd_window_f32(F, F, F, F, SY, LO, HI, ex, F, nullptr, ws, sizeof ws, 8, 1000, 64, 5, 99, nullptr, nullptr), NW_ERR_UNSUPPORTED);
        EXPECT(nw_fwd_window_f32(F, F, F, F, SY, LO, HI, ex, F, nullptr, ws, sizeof ws, 8, 1000, 100, 5, E, nullptr, nullptr), NW_ERR_UNSUPPORTED);
        EXPECT(nw_fwd_window_f32(F, F, F, F, SY, LO, HI, ex, F, nullptr, ws, sizeof ws, 8, 1000, 16, 5, E, nullptr, nullptr), NW_ERR_UNSUPPORTED);
        EXPECT(nw_fwd_window_f32(F, F, F, F, SY, LO, HI, ex, F, nullptr, ws, sizeof ws, 8, 1000, 0, 5, E, nullptr, nullptr), NW_ERR_UNSUPPORTED);
        EXPECT(nw_fwd_window_f32(F, F, F, F, SY, LO, HI, ex, F, nullptr, ws, sizeof ws, 8, 25, 64, 5, E, nullptr, nullptr), NW_ERR_UNSUPPORTED);
        EXPECT(nw_fwd_window_f32(F, F, F, F, SY, LO, HI, ex, F, nullptr, ws, sizeof ws, 8, 0, 64, 5, E, nullptr, nullptr), NW_ERR_UNSUPPORTED);
        EXPECT(nw_fwd_window_f32(F, F, F, F, SY, LO, HI, ex, F, nullptr, ws, sizeof ws, 8, 1000, 64, 0, E, nullptr, nullptr), NW_ERR_UNSUPPORTED);
        EXPECT(nw_fwd_window_f32(F, F, F, F, SY, LO, HI, ex, F, nullptr, ws, sizeof ws, 8, 1000, 64, 50000, E, nullptr, nullptr), NW_ERR_UNSUPPORTED);
        EXPECT(nw_fwd_window_f32(F + 1, F, F, F, SY, LO, HI, ex, F, nullptr, ws, sizeof ws, 8, 1000, 64, 5, E, nullptr, nullptr), NW_ERR_UNSUPPORTED);
        EXPECT(nw_fwd_window_f32(F, F + 1, F, F, SY, LO, HI, ex, F, nullptr, ws, sizeof ws, 8, 1000, 64, 5, E, nullptr, nullptr), NW_ERR_UNSUPPORTED);
        // the workspace
        EXPECT(nw_fwd_window_f32(F, F, F, F, SY, LO, HI, ex, F, nullptr, ws, sizeof ws, 8, 1000, 64, 5, E, nullptr, nullptr), NW_ERR_WORKSPACE);
        EXPECT(nw_fwd_window_f32(F, F, F, F, SY, LO, HI, ex, F, nullptr, nullptr, 0, 8, 1000, 64, 5, E, nullptr, nullptr), NW_ERR_WORKSPACE);
        EXPECT(nw_fwd_window_f32(F, F, F, F, SY, LO, HI, ex, F, F, ws, need - 1, 8, 1000, 64, 5, E, nullptr, nullptr), NW_ERR_WORKSPACE);
        EXPECT(nw_fwd_window_f32(F, F, F, F, SY, LO, HI, ex, F, nullptr, ws + 4, need, 8, 1000, 64, 5, E, nullptr, nullptr), NW_ERR_UNSUPPORTED);
        // B == 0 with a window: NW_OK, nothing is read, nothing is launched
        EXPECT(nw_fwd_window_f32(nullptr, nullptr, nullptr, nullptr, nullptr, LO, HI, ex, nullptr, nullptr, nullptr, 0, 0, 1000, 64, 5, E, nullptr,
                                 nullptr), NW_OK);
    }
    std::printf(failures ? "abi_args_fwd_window: %d FAILED\n" : "abi_args_fwd_window: all argument checks refused as documented\n",
                failures);
    return failures ? 1 : 0;
}
