// Host-only exercise of nw_fwd_weighted_f32 and nw_bwd_query_weighted_f32 (include/nwhead_hip.h) under AddressSanitizer +
// UndefinedBehaviorSanitizer, like abi_args_fwd_window.cpp / abi_args_bwd_query.cpp: built by
// `make -C nwhead_amd/csrc sanitize_fwd_weighted` from the library's own sources with --cuda-host-only against
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
    std::vector<int64_t> lab(64, 0);
    std::vector<int32_t> win(64, 0);
    const int64_t* SY = lab.data();
    const int32_t *LO = win.data(), *HI = win.data() + 32;
    const int E = NW_SCORE_EUCLIDEAN;
    const size_t need = nw_fwd_workspace_bytes(8, 1000, 64, 5);
    const size_t bneed = nw_bwd_query_workspace_bytes(8, 1000, 64, 5, 0);
    EXPECT(need > 0, 1);
    EXPECT(bneed > 0, 1);

    // ================================ nw_fwd_weighted_f32
#define FWD(q, s, sy, a, lo, hi, ex, out, wsp, wsb, B, N, d, C, kind) \
    nw_fwd_weighted_f32(q, s, F, F, sy, a, lo, hi, ex, out, nullptr, wsp, wsb, B, N, d, C, kind, nullptr, nullptr)
    // the weights are required; the window is both arrays or neither
    EXPECT(FWD(F, F, SY, nullptr, LO, HI, 0, F, ws, sizeof ws, 8, 1000, 64, 5, E), NW_ERR_INVALID_ARG);
    EXPECT(FWD(F, F, SY, nullptr, nullptr, nullptr, 0, F, ws, sizeof ws, 8, 1000, 64, 5, E), NW_ERR_INVALID_ARG);
    EXPECT(FWD(F, F, SY, F, nullptr, HI, 0, F, ws, sizeof ws, 8, 1000, 64, 5, E), NW_ERR_INVALID_ARG);
    EXPECT(FWD(F, F, SY, F, LO, nullptr, 1, F, ws, sizeof ws, 8, 1000, 64, 5, E), NW_ERR_INVALID_ARG);
    for (int windowed = 0; windowed < 2; ++windowed) {
        const int32_t *lo = windowed ? LO : nullptr, *hi = windowed ? HI : nullptr;
        for (int ex = 0; ex < 2; ++ex) {
            // negative sizes, null operands, clip without its scale
            EXPECT(FWD(F, F, SY, F, lo, hi, ex, F, ws, sizeof ws, -1, 1000, 64, 5, E), NW_ERR_INVALID_ARG);
            EXPECT(FWD(F, F, SY, F, lo, hi, ex, F, ws, sizeof ws, 8, -1, 64, 5, E), NW_ERR_INVALID_ARG);
            EXPECT(FWD(F, F, SY, F, lo, hi, ex, F, ws, sizeof ws, 8, 1000, -64, 5, E), NW_ERR_INVALID_ARG);
            EXPECT(FWD(F, F, SY, F, lo, hi, ex, F, ws, sizeof ws, 8, 1000, 64, -5, E), NW_ERR_INVALID_ARG);
            EXPECT(FWD(nullptr, F, SY, F, lo, hi, ex, F, ws, sizeof ws, 8, 1000, 64, 5, E), NW_ERR_INVALID_ARG);
            EXPECT(FWD(F, nullptr, SY, F, lo, hi, ex, F, ws, sizeof ws, 8, 1000, 64, 5, E), NW_ERR_INVALID_ARG);
            EXPECT(FWD(F, F, nullptr, F, lo, hi, ex, F, ws, sizeof ws, 8, 1000, 64, 5, E), NW_ERR_INVALID_ARG);
            EXPECT(FWD(F, F, SY, F, lo, hi, ex, nullptr, ws, sizeof ws, 8, 1000, 64, 5, E), NW_ERR_INVALID_ARG);
            EXPECT(FWD(F, F, SY, F, lo, hi, ex, F, ws, sizeof ws, 8, 1000, 64, 5, NW_SCORE_CLIP), NW_ERR_INVALID_ARG);
            // outside the regime of nw_fwd_window_f32
            EXPECT(FWD(F, F, SY, F, lo, hi, ex, F, ws, sizeof ws, 8, 1000, 64, 5, 99), NW_ERR_UNSUPPORTED);
            EXPECT(FWD(F, F, SY, F, lo, hi, ex, F, ws, sizeof ws, 8, 1000, 100, 5, E), NW_ERR_UNSUPPORTED);
            EXPECT(FWD(F, F, SY, F, lo, hi, ex, F, ws, sizeof ws, 8, 1000, 16, 5, E), NW_ERR_UNSUPPORTED);
            EXPECT(FWD(F, F, SY, F, lo, hi, ex, F, ws, sizeof ws, 8, 25, 64, 5, E), NW_ERR_UNSUPPORTED);
            EXPECT(FWD(F, F, SY, F, lo, hi, ex, F, ws, sizeof ws, 8, 1000, 64, 0, E), NW_ERR_UNSUPPORTED);
            EXPECT(FWD(F, F, SY, F, lo, hi, ex, F, ws, sizeof ws, 8, 1000, 64, 50000, E), NW_ERR_UNSUPPORTED);
            EXPECT(FWD(F + 1, F, SY, F, lo, hi, ex, F, ws, sizeof ws, 8, 1000, 64, 5, E), NW_ERR_UNSUPPORTED);
            EXPECT(FWD(F, F + 1, SY, F, lo, hi, ex, F, ws, sizeof ws, 8, 1000, 64, 5, E), NW_ERR_UNSUPPORTED);
            EXPECT(FWD(F, F, SY, F + 1, lo, hi, ex, F, ws, sizeof ws, 8, 1000, 64, 5, E), NW_ERR_UNSUPPORTED);   // the weights' alignment
            // the workspace
            EXPECT(FWD(F, F, SY, F, lo, hi, ex, F, ws, sizeof ws, 8, 1000, 64, 5, E), NW_ERR_WORKSPACE);
            EXPECT(FWD(F, F, SY, F, lo, hi, ex, F, nullptr, 0, 8, 1000, 64, 5, E), NW_ERR_WORKSPACE);
            EXPECT(FWD(F, F, SY, F, lo, hi, ex, F, ws, need - 1, 8, 1000, 64, 5, E), NW_ERR_WORKSPACE);
            EXPECT(FWD(F, F, SY, F, lo, hi, ex, F, ws + 4, need, 8, 1000, 64, 5, E), NW_ERR_UNSUPPORTED);
            // B == 0: NW_OK, nothing is read, nothing is launched
            EXPECT(FWD(nullptr, nullptr, nullptr, nullptr, lo, hi, ex, nullptr, nullptr, 0, 0, 1000, 64, 5, E), NW_OK);
        }
    }

    // ================================ nw_bwd_query_weighted_f32
#define BWD(q, s, sy, a, lo, hi, ex, lse, out, gout, gq, wsp, wsb, B, N, d, C, kind, chunks) \
    nw_bwd_query_weighted_f32(q, s, F, F, sy, a, lo, hi, ex, lse, out, gout, gq, nullptr, wsp, wsb, B, N, d, C, kind, nullptr, chunks, nullptr)
    EXPECT(BWD(F, F, SY, nullptr, LO, HI, 0, F, F, F, F, ws, sizeof ws, 8, 1000, 64, 5, E, 0), NW_ERR_INVALID_ARG);
    EXPECT(BWD(F, F, SY, F, LO, nullptr, 0, F, F, F, F, ws, sizeof ws, 8, 1000, 64, 5, E, 0), NW_ERR_INVALID_ARG);
    EXPECT(BWD(F, F, SY, F, nullptr, HI, 1, F, F, F, F, ws, sizeof ws, 8, 1000, 64, 5, E, 0), NW_ERR_INVALID_ARG);
    for (int windowed = 0; windowed < 2; ++windowed) {
        const int32_t *lo = windowed ? LO : nullptr, *hi = windowed ? HI : nullptr;
        for (int ex = 0; ex < 2; ++ex) {
            EXPECT(BWD(F, F, SY, F, lo, hi, ex, F, F, F, F, ws, sizeof ws, -1, 1000, 64, 5, E, 0), NW_ERR_INVALID_ARG);
            EXPECT(BWD(F, F, SY, F, lo, hi, ex, F, F, F, F, ws, sizeof ws, 8, 1000, 64, 5, E, -1), NW_ERR_INVALID_ARG);
            EXPECT(BWD(nullptr, F, SY, F, lo, hi, ex, F, F, F, F, ws, sizeof ws, 8, 1000, 64, 5, E, 0), NW_ERR_INVALID_ARG);
            EXPECT(BWD(F, F, nullptr, F, lo, hi, ex, F, F, F, F, ws, sizeof ws, 8, 1000, 64, 5, E, 0), NW_ERR_INVALID_ARG);
            EXPECT(BWD(F, F, SY, F, lo, hi, ex, nullptr, F, F, F, ws, sizeof ws, 8, 1000, 64, 5, E, 0), NW_ERR_INVALID_ARG);
            EXPECT(BWD(F, F, SY, F, lo, hi, ex, F, nullptr, F, F, ws, sizeof ws, 8, 1000, 64, 5, E, 0), NW_ERR_INVALID_ARG);
            EXPECT(BWD(F, F, SY, F, lo, hi, ex, F, F, nullptr, F, ws, sizeof ws, 8, 1000, 64, 5, E, 0), NW_ERR_INVALID_ARG);
            EXPECT(BWD(F, F, SY, F, lo, hi, ex, F, F, F, nullptr, ws, sizeof ws, 8, 1000, 64, 5, E, 0), NW_ERR_INVALID_ARG);
            EXPECT(BWD(F, F, SY, F, lo, hi, ex, F, F, F, F, ws, sizeof ws, 8, 1000, 64, 5, NW_SCORE_CLIP, 0), NW_ERR_INVALID_ARG);
            EXPECT(BWD(F, F, SY, F, lo, hi, ex, F, F, F, F, ws, sizeof ws, 8, 1000, 64, 5, 99, 0), NW_ERR_UNSUPPORTED);
            EXPECT(BWD(F, F, SY, F, lo, hi, ex, F, F, F, F, ws, sizeof ws, 8, 1000, 100, 5, E, 0), NW_ERR_UNSUPPORTED);
            EXPECT(BWD(F, F, SY, F, lo, hi, ex, F, F, F, F, ws, sizeof ws, 8, 25, 64, 5, E, 0), NW_ERR_UNSUPPORTED);
            EXPECT(BWD(F, F, SY, F, lo, hi, ex, F, F, F, F, ws, sizeof ws, 8, 1000, 64, 0, E, 0), NW_ERR_UNSUPPORTED);
            EXPECT(BWD(F + 1, F, SY, F, lo, hi, ex, F, F, F, F, ws, sizeof ws, 8, 1000, 64, 5, E, 0), NW_ERR_UNSUPPORTED);
            EXPECT(BWD(F, F, SY, F, lo, hi, ex, F, F, F, F + 1, ws, sizeof ws, 8, 1000, 64, 5, E, 0), NW_ERR_UNSUPPORTED);
            EXPECT(BWD(F, F, SY, F + 1, lo, hi, ex, F, F, F, F, ws, sizeof ws, 8, 1000, 64, 5, E, 0), NW_ERR_UNSUPPORTED);
            EXPECT(BWD(F, F, SY, F, lo, hi, ex, F, F, F, F, ws, sizeof ws, 8, 1000, 64, 5, E, 0), NW_ERR_WORKSPACE);
            EXPECT(BWD(F, F, SY, F, lo, hi, ex, F, F, F, F, nullptr, bneed, 8, 1000, 64, 5, E, 0), NW_ERR_WORKSPACE);
            EXPECT(BWD(F, F, SY, F, lo, hi, ex, F, F, F, F, ws, bneed - 1, 8, 1000, 64, 5, E, 0), NW_ERR_WORKSPACE);
            EXPECT(BWD(F, F, SY, F, lo, hi, ex, F, F, F, F, ws + 4, bneed, 8, 1000, 64, 5, E, 0), NW_ERR_UNSUPPORTED);
            EXPECT(BWD(nullptr, nullptr, nullptr, nullptr, lo, hi, ex, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, 1000, 64, 5, E, 0), NW_OK);
        }
    }
    std::printf(failures ? "abi_args_fwd_weighted: %d FAILED\n" : "abi_args_fwd_weighted: all argument checks refused as documented\n",
                failures);
    return failures ? 1 : 0;
}
