// Host-only exercise of nw_knn_window_f32 / nw_influence_select_f32 (include/nwhead_hip.h) under AddressSanitizer +
// UndefinedBehaviorSanitizer, like abi_args_knn_f16.cpp: built by `make -C nwhead_amd/csrc sanitize_knn_window` from the
// library's own sources with --cuda-host-only against hip_stubs.cpp.  Every call here is a pure host computation or must
// be refused BEFORE anything is launched, with the documented status and without a sanitizer report.
#include <cstdint>
#include <cstdio>
#include <vector>
#include "../../include/nwhead_hip.h"
#include "expect.h"

int main() {
    alignas(16) static float F[4096];
    alignas(16) static char ws[256];
    std::vector<int64_t> idx(64, 0);
    std::vector<int32_t> win(64, 0);
    int64_t* I = idx.data();
    const int32_t *LO = win.data(), *HI = win.data() + 32;
    const int E = NW_SCORE_EUCLIDEAN;
    // ---- the windowed search takes nw_knn_f32's workspace
    const size_t need = nw_knn_workspace_bytes(8, 1000, 64, 10);
    EXPECT(need > 0, 1);
    // ---- refused before any launch: the window itself
    EXPECT(nw_knn_window_f32(F, F, F, F, nullptr, HI, 0, I, nullptr, ws, sizeof ws, 8, 1000, 64, 10, E, nullptr, nullptr), NW_ERR_INVALID_ARG);
    EXPECT(nw_knn_window_f32(F, F, F, F, LO, nullptr, 0, I, nullptr, ws, sizeof ws, 8, 1000, 64, 10, E, nullptr, nullptr), NW_ERR_INVALID_ARG);
    EXPECT(nw_knn_window_f32(F, F, F, F, nullptr, nullptr, 1, I, nullptr, ws, sizeof ws, 8, 1000, 64, 10, E, nullptr, nullptr), NW_ERR_INVALID_ARG);
    EXPECT(nw_knn_window_f32(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0, 0, 1000, 64, 10, E,
                             nullptr, nullptr), NW_ERR_INVALID_ARG);                                  // ... even with B == 0
    // ---- ... and everything nw_knn_f32 refuses, inside and excluded
    for (int ex = 0; ex < 2; ++ex) {
        EXPECT(nw_knn_window_f32(F, F, F, F, LO, HI, ex, I, nullptr, ws, sizeof ws, -1, 1000, 64, 10, E, nullptr, nullptr), NW_ERR_INVALID_ARG);
        EXPECT(nw_knn_window_f32(F, F, F, F, LO, HI, ex, I, nullptr, ws, sizeof ws, 8, -1, 64, 10, E, nullptr, nullptr), NW_ERR_INVALID_ARG);
        EXPECT(nw_knn_window_f32(F, F, F, F, LO, HI, ex, I, nullptr, ws, sizeof ws, 8, 1000, -64, 10, E, nullptr, nullptr), NW_ERR_INVALID_ARG);
        EXPECT(nw_knn_window_f32(F, F, F, F, LO, HI, ex, I, nullptr, ws, sizeof ws, 8, 1000, 64, 10, 99, nullptr, nullptr), NW_ERR_UNSUPPORTED);
        EXPECT(nw_knn_window_f32(nullptr, F, F, F, LO, HI, ex, I, nullptr, ws, sizeof ws, 8, 1000, 64, 10, E, nullptr, nullptr), NW_ERR_INVALID_ARG);
        EXPECT(nw_knn_window_f32(F, nullptr, F, F, LO, HI, ex, I, nullptr, ws, sizeof ws, 8, 1000, 64, 10, E, nullptr, nullptr), NW_ERR_INVALID_ARG);
        EXPECT(nw_knn_window_f32(F, F, nullptr, F, LO, HI, ex, I, nullptr, ws, sizeof ws, 8, 1000, 64, 10, E, nullptr, nullptr), NW_ERR_INVALID_ARG);
        EXPECT(nw_knn_window_f32(F, F, F, nullptr, LO, HI, ex, I, nullptr, ws, sizeof ws, 8, 1000, 64, 10, E, nullptr, nullptr), NW_ERR_INVALID_ARG);
        EXPECT(nw_knn_window_f32(F, F, F, F, LO, HI, ex, nullptr, nullptr, ws, sizeof ws, 8, 1000, 64, 10, E, nullptr, nullptr), NW_ERR_INVALID_ARG);
        EXPECT(nw_knn_window_f32(F, F, F, F, LO, HI, ex, I, nullptr, ws, sizeof ws, 8, 1000, 64, 10, NW_SCORE_CLIP, nullptr, nullptr),
               NW_ERR_INVALID_ARG);                                                                   // clip without logit_scale
        EXPECT(nw_knn_window_f32(F + 1, F, F, F, LO, HI, ex, I, nullptr, ws, sizeof ws, 8, 1000, 64, 10, E, nullptr, nullptr), NW_ERR_INVALID_ARG);
        EXPECT(nw_knn_window_f32(F, F + 1, F, F, LO, HI, ex, I, nullptr, ws, sizeof ws, 8, 1000, 64, 10, E, nullptr, nullptr), NW_ERR_INVALID_ARG);
        EXPECT(nw_knn_window_f32(F, F, F, F, LO, HI, ex, I, nullptr, ws + 4, sizeof ws - 4, 8, 1000, 64, 10, E, nullptr, nullptr), NW_ERR_INVALID_ARG);
        EXPECT(nw_knn_window_f32(F, F, F, F, LO, HI, ex, I, nullptr, ws, sizeof ws, 8, 1000, 100, 10, E, nullptr, nullptr), NW_ERR_UNSUPPORTED);
        EXPECT(nw_knn_window_f32(F, F, F, F, LO, HI, ex, I, nullptr, ws, sizeof ws, 8, 1000, 64, 33, E, nullptr, nullptr), NW_ERR_UNSUPPORTED);
        EXPECT(nw_knn_window_f32(F, F, F, F, LO, HI, ex, I, nullptr, ws, sizeof ws, 8, 1000, 64, 0, E, nullptr, nullptr), NW_ERR_UNSUPPORTED);
        EXPECT(nw_knn_window_f32(F, F, F, F, LO, HI, ex, I, nullptr, ws, sizeof ws, 8, 20, 64, 5, E, nullptr, nullptr), NW_ERR_UNSUPPORTED);
        EXPECT(nw_knn_window_f32(F, F, F, F, LO, HI, ex, I, nullptr, ws, sizeof ws, 8, 30, 64, 31, E, nullptr, nullptr), NW_ERR_UNSUPPORTED);
        EXPECT(nw_knn_window_f32(F, F, F, F, LO, HI, ex, I, nullptr, ws, sizeof ws, 8, 0, 64, 10, E, nullptr, nullptr), NW_ERR_UNSUPPORTED);
        EXPECT(nw_knn_window_f32(F, F, F, F, LO, HI, ex, I, nullptr, ws, sizeof ws, 8, 1000, 64, 10, E, nullptr, nullptr), NW_ERR_WORKSPACE);
        EXPECT(nw_knn_window_f32(F, F, F, F, LO, HI, ex, I, nullptr, nullptr, 0, 8, 1000, 64, 10, E, nullptr, nullptr), NW_ERR_WORKSPACE);
        EXPECT(nw_knn_window_f32(F, F, F, F, LO, HI, ex, I, nullptr, ws, need - 1, 8, 1000, 64, 10, E, nullptr, nullptr), NW_ERR_WORKSPACE);
        // B == 0 with a window: NW_OK, nothing is read, nothing is launched
        EXPECT(nw_knn_window_f32(nullptr, nullptr, nullptr, nullptr, LO, HI, ex, nullptr, nullptr, nullptr, 0, 0, 1000, 64, 10, E, nullptr,
                                 nullptr), NW_OK);
    }
    // ---- nw_influence_select_f32
    const int64_t *R = I, *SY = I, *QY = I;
    EXPECT(nw_influence_select_f32(F, R, SY, QY, F, F, F, nullptr, -1, 10, 100, 5, nullptr), NW_ERR_INVALID_ARG);
    EXPECT(nw_influence_select_f32(F, R, SY, QY, F, F, F, nullptr, 4, -1, 100, 5, nullptr), NW_ERR_INVALID_ARG);
    EXPECT(nw_influence_select_f32(F, R, SY, QY, F, F, F, nullptr, 4, 10, -1, 5, nullptr), NW_ERR_INVALID_ARG);
    EXPECT(nw_influence_select_f32(F, R, SY, QY, F, F, F, nullptr, 4, 10, 100, -1, nullptr), NW_ERR_INVALID_ARG);
    EXPECT(nw_influence_select_f32(nullptr, R, SY, QY, F, F, F, nullptr, 4, 10, 100, 5, nullptr), NW_ERR_INVALID_ARG);
    EXPECT(nw_influence_select_f32(F, nullptr, SY, QY, F, F, F, nullptr, 4, 10, 100, 5, nullptr), NW_ERR_INVALID_ARG);
    EXPECT(nw_influence_select_f32(F, R, nullptr, QY, F, F, F, nullptr, 4, 10, 100, 5, nullptr), NW_ERR_INVALID_ARG);
    EXPECT(nw_influence_select_f32(F, R, SY, nullptr, F, F, F, nullptr, 4, 10, 100, 5, nullptr), NW_ERR_INVALID_ARG);
    EXPECT(nw_influence_select_f32(F, R, SY, QY, nullptr, F, F, nullptr, 4, 10, 100, 5, nullptr), NW_ERR_INVALID_ARG);
    EXPECT(nw_influence_select_f32(F, R, SY, QY, F, nullptr, F, nullptr, 4, 10, 100, 5, nullptr), NW_ERR_INVALID_ARG);
    EXPECT(nw_influence_select_f32(F, R, SY, QY, F, F, nullptr, nullptr, 4, 10, 100, 5, nullptr), NW_ERR_INVALID_ARG);
    EXPECT(nw_influence_select_f32(F, R, SY, QY, F, F, nullptr, I, 4, 10, 100, 5, nullptr), NW_ERR_INVALID_ARG);
    EXPECT(nw_influence_select_f32(F, R, SY, QY, F, F, F, nullptr, 4, 0, 100, 5, nullptr), NW_ERR_UNSUPPORTED);
    EXPECT(nw_influence_select_f32(F, R, SY, QY, F, F, F, nullptr, 4, 33, 100, 5, nullptr), NW_ERR_UNSUPPORTED);
    EXPECT(nw_influence_select_f32(F, R, SY, QY, F, F, F, I, 4, 1024, 100, 5, nullptr), NW_ERR_UNSUPPORTED);
    EXPECT(nw_influence_select_f32(F, R, SY, QY, F, F, F, nullptr, (int64_t)1 << 31, 10, 100, 5, nullptr), NW_ERR_UNSUPPORTED);
    EXPECT(nw_influence_select_f32(F, R, SY, QY, F, F, F, nullptr, 0, 10, 100, 5, nullptr), NW_OK);   // nothing to do
    EXPECT(nw_influence_select_f32(F, R, SY, QY, F, F, F, I, 0, 32, 0, 0, nullptr), NW_OK);
    std::printf(failures ? "abi_args_knn_window: %d FAILED\n" : "abi_args_knn_window: all argument checks refused as documented\n",
                failures);
    return failures ? 1 : 0;
}
