// Host-only exercise of nw_bwd_values_support_f32 and nw_bwd_values_support_workspace_bytes (include/nwhead_hip.h) under
// AddressSanitizer + UndefinedBehaviorSanitizer, like abi_args_bwd_values.cpp: built by
// `make -C nwhead_amd/csrc sanitize_bwd_values_support` from the library's own sources with --cuda-host-only against
// hip_stubs.cpp.  Every call here must be refused BEFORE anything is launched (or, with B == 0, answered), with the
// documented status and without a sanitizer report.
#include <cstdint>
#include <cstdio>
#include <vector>
#include "../../include/nwhead_hip.h"
#include "expect.h"

int main() {
    alignas(16) static float F[4096];
    alignas(16) static char ws[256];
    std::vector<int32_t> win(64, 0);
    const int32_t *LO = win.data(), *HI = win.data() + 32;
    const int E = NW_SCORE_EUCLIDEAN;
    const size_t need = nw_bwd_values_support_workspace_bytes(8, 1000, 64, 32, 0, 1);
    EXPECT(need > 0, 1);
    EXPECT(nw_bwd_values_support_workspace_bytes(8, 1000, 64, 32, 0, 0) > 0, 1);
    // forced query chunks with gvalues size the partial tiles; without gvalues nothing of size N x T
    EXPECT(nw_bwd_values_support_workspace_bytes(200, 1000, 64, 64, 3, 1) > nw_bwd_values_support_workspace_bytes(200, 1000, 64, 64, 1, 1), 1);
    EXPECT(nw_bwd_values_support_workspace_bytes(200, 1000, 64, 64, 3, 0) < (size_t)1000 * 64 * 4, 1);
    // outside the regime, or nothing to do: 0
    EXPECT(nw_bwd_values_support_workspace_bytes(0, 1000, 64, 32, 0, 1), 0);
    EXPECT(nw_bwd_values_support_workspace_bytes(-1, 1000, 64, 32, 0, 1), 0);
    EXPECT(nw_bwd_values_support_workspace_bytes(8, 25, 64, 32, 0, 1), 0);
    EXPECT(nw_bwd_values_support_workspace_bytes(8, 1000, 100, 32, 0, 1), 0);
    EXPECT(nw_bwd_values_support_workspace_bytes(8, 1000, 16, 32, 0, 1), 0);
    EXPECT(nw_bwd_values_support_workspace_bytes(8, 1000, 64, 0, 0, 1), 0);
    EXPECT(nw_bwd_values_support_workspace_bytes(8, 1000, 64, 5, 0, 1), 0);
    EXPECT(nw_bwd_values_support_workspace_bytes(8, 1000, 64, 16384 + 32, 0, 1), 0);
    EXPECT(nw_bwd_values_support_workspace_bytes(8, 1000, 64, 32, -1, 1), 0);
    EXPECT(nw_bwd_values_support_workspace_bytes(8, 1000, 64, 16384, 0, 1) > 0, 1);

#define SUP(q, s, v, a, lo, hi, ex, lse, out, gout, gv, ga, wsp, wsb, B, N, d, T, kind, chunks) \
    nw_bwd_values_support_f32(q, s, F, F, v, a, lo, hi, ex, lse, out, gout, gv, ga, wsp, wsb, B, N, d, T, kind, nullptr, chunks, nullptr)
    // the window is both arrays or neither
    EXPECT(SUP(F, F, F, F, nullptr, HI, 0, F, F, F, F, F, ws, sizeof ws, 8, 1000, 64, 32, E, 0), NW_ERR_INVALID_ARG);
    EXPECT(SUP(F, F, F, F, LO, nullptr, 1, F, F, F, F, F, ws, sizeof ws, 8, 1000, 64, 32, E, 0), NW_ERR_INVALID_ARG);
    // at least one result; glogw needs the weights and the value rows
    EXPECT(SUP(F, F, F, F, LO, HI, 0, F, F, F, nullptr, nullptr, ws, sizeof ws, 8, 1000, 64, 32, E, 0), NW_ERR_INVALID_ARG);
    EXPECT(SUP(F, F, F, nullptr, LO, HI, 0, F, F, F, F, F, ws, sizeof ws, 8, 1000, 64, 32, E, 0), NW_ERR_INVALID_ARG);
    EXPECT(SUP(F, F, nullptr, F, LO, HI, 0, F, F, F, F, F, ws, sizeof ws, 8, 1000, 64, 32, E, 0), NW_ERR_INVALID_ARG);
    EXPECT(SUP(F, F, nullptr, F, LO, HI, 0, F, F, F, nullptr, F, ws, sizeof ws, 8, 1000, 64, 32, E, 0), NW_ERR_INVALID_ARG);
    // ... gvalues alone needs neither: the call gets as far as the workspace
    EXPECT(SUP(F, F, nullptr, nullptr, LO, HI, 0, F, F, F, F, nullptr, ws, sizeof ws, 8, 1000, 64, 32, E, 0), NW_ERR_WORKSPACE);
    for (int mode = 0; mode < 3; ++mode) {            // gvalues and glogw, gvalues alone, the weights-only mode
        float* gv = mode < 2 ? F : nullptr;
        float* ga = mode != 1 ? F : nullptr;
        const float* a = mode != 1 ? F : nullptr;
        const size_t mneed = nw_bwd_values_support_workspace_bytes(8, 1000, 64, 32, 0, gv != nullptr);
        for (int windowed = 0; windowed < 2; ++windowed) {
            const int32_t *lo = windowed ? LO : nullptr, *hi = windowed ? HI : nullptr;
            for (int ex = 0; ex < 2; ++ex) {
                // negative sizes, null operands, clip without its scale
                EXPECT(SUP(F, F, F, a, lo, hi, ex, F, F, F, gv, ga, ws, sizeof ws, -1, 1000, 64, 32, E, 0), NW_ERR_INVALID_ARG);
                EXPECT(SUP(F, F, F, a, lo, hi, ex, F, F, F, gv, ga, ws, sizeof ws, 8, -1, 64, 32, E, 0), NW_ERR_INVALID_ARG);
                EXPECT(SUP(F, F, F, a, lo, hi, ex, F, F, F, gv, ga, ws, sizeof ws, 8, 1000, -64, 32, E, 0), NW_ERR_INVALID_ARG);
                EXPECT(SUP(F, F, F, a, lo, hi, ex, F, F, F, gv, ga, ws, sizeof ws, 8, 1000, 64, -32, E, 0), NW_ERR_INVALID_ARG);
                EXPECT(SUP(F, F, F, a, lo, hi, ex, F, F, F, gv, ga, ws, sizeof ws, 8, 1000, 64, 32, E, -1), NW_ERR_INVALID_ARG);
                EXPECT(SUP(nullptr, F, F, a, lo, hi, ex, F, F, F, gv, ga, ws, sizeof ws, 8, 1000, 64, 32, E, 0), NW_ERR_INVALID_ARG);
                EXPECT(SUP(F, nullptr, F, a, lo, hi, ex, F, F, F, gv, ga, ws, sizeof ws, 8, 1000, 64, 32, E, 0), NW_ERR_INVALID_ARG);
                EXPECT(SUP(F, F, F, a, lo, hi, ex, nullptr, F, F, gv, ga, ws, sizeof ws, 8, 1000, 64, 32, E, 0), NW_ERR_INVALID_ARG);
                EXPECT(SUP(F, F, F, a, lo, hi, ex, F, nullptr, F, gv, ga, ws, sizeof ws, 8, 1000, 64, 32, E, 0), NW_ERR_INVALID_ARG);
                EXPECT(SUP(F, F, F, a, lo, hi, ex, F, F, nullptr, gv, ga, ws, sizeof ws, 8, 1000, 64, 32, E, 0), NW_ERR_INVALID_ARG);
                EXPECT(SUP(F, F, F, a, lo, hi, ex, F, F, F, gv, ga, ws, sizeof ws, 8, 1000, 64, 32, NW_SCORE_CLIP, 0), NW_ERR_INVALID_ARG);
                // outside the regime
                EXPECT(SUP(F, F, F, a, lo, hi, ex, F, F, F, gv, ga, ws, sizeof ws, 8, 1000, 64, 32, 99, 0), NW_ERR_UNSUPPORTED);
                EXPECT(SUP(F, F, F, a, lo, hi, ex, F, F, F, gv, ga, ws, sizeof ws, 8, 1000, 100, 32, E, 0), NW_ERR_UNSUPPORTED);
                EXPECT(SUP(F, F, F, a, lo, hi, ex, F, F, F, gv, ga, ws, sizeof ws, 8, 1000, 16, 32, E, 0), NW_ERR_UNSUPPORTED);
                EXPECT(SUP(F, F, F, a, lo, hi, ex, F, F, F, gv, ga, ws, sizeof ws, 8, 25, 64, 32, E, 0), NW_ERR_UNSUPPORTED);
                EXPECT(SUP(F, F, F, a, lo, hi, ex, F, F, F, gv, ga, ws, sizeof ws, 8, 1000, 64, 0, E, 0), NW_ERR_UNSUPPORTED);
                EXPECT(SUP(F, F, F, a, lo, hi, ex, F, F, F, gv, ga, ws, sizeof ws, 8, 1000, 64, 5, E, 0), NW_ERR_UNSUPPORTED);
                EXPECT(SUP(F, F, F, a, lo, hi, ex, F, F, F, gv, ga, ws, sizeof ws, 8, 1000, 64, 16384 + 32, E, 0), NW_ERR_UNSUPPORTED);
                EXPECT(SUP(F + 1, F, F, a, lo, hi, ex, F, F, F, gv, ga, ws, sizeof ws, 8, 1000, 64, 32, E, 0), NW_ERR_UNSUPPORTED);
                EXPECT(SUP(F, F + 1, F, a, lo, hi, ex, F, F, F, gv, ga, ws, sizeof ws, 8, 1000, 64, 32, E, 0), NW_ERR_UNSUPPORTED);
                EXPECT(SUP(F, F, F + 1, a, lo, hi, ex, F, F, F, gv, ga, ws, sizeof ws, 8, 1000, 64, 32, E, 0), NW_ERR_UNSUPPORTED);
                EXPECT(SUP(F, F, F, a, lo, hi, ex, F, F, F + 1, gv, ga, ws, sizeof ws, 8, 1000, 64, 32, E, 0), NW_ERR_UNSUPPORTED);
                if (gv) EXPECT(SUP(F, F, F, a, lo, hi, ex, F, F, F, F + 1, ga, ws, sizeof ws, 8, 1000, 64, 32, E, 0), NW_ERR_UNSUPPORTED);
                if (ga) EXPECT(SUP(F, F, F, a, lo, hi, ex, F, F, F, gv, F + 1, ws, sizeof ws, 8, 1000, 64, 32, E, 0), NW_ERR_UNSUPPORTED);
                if (a) EXPECT(SUP(F, F, F, F + 1, lo, hi, ex, F, F, F, gv, ga, ws, sizeof ws, 8, 1000, 64, 32, E, 0), NW_ERR_UNSUPPORTED);
                // the workspace
                EXPECT(SUP(F, F, F, a, lo, hi, ex, F, F, F, gv, ga, ws, sizeof ws, 8, 1000, 64, 32, E, 0), NW_ERR_WORKSPACE);
                EXPECT(SUP(F, F, F, a, lo, hi, ex, F, F, F, gv, ga, nullptr, mneed, 8, 1000, 64, 32, E, 0), NW_ERR_WORKSPACE);
                EXPECT(SUP(F, F, F, a, lo, hi, ex, F, F, F, gv, ga, ws, mneed - 1, 8, 1000, 64, 32, E, 0), NW_ERR_WORKSPACE);
                EXPECT(SUP(F, F, F, a, lo, hi, ex, F, F, F, gv, ga, ws + 4, mneed, 8, 1000, 64, 32, E, 0), NW_ERR_UNSUPPORTED);
                // B == 0: NW_OK, nothing is read, nothing is launched, nothing is written
                EXPECT(SUP(nullptr, nullptr, nullptr, nullptr, lo, hi, ex, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, 1000,
                           64, 32, E, 0), NW_OK);
            }
        }
    }
    std::printf(failures ? "abi_args_bwd_values_support: %d FAILED\n"
                         : "abi_args_bwd_values_support: all argument checks refused as documented\n",
                failures);
    return failures ? 1 : 0;
}
