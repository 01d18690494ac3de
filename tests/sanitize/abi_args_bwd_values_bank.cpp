// Host-only exercise of nw_bwd_values_bank_support_f32 and nw_bwd_values_bank_support_workspace_bytes
// (include/nwhead_hip.h) under AddressSanitizer + UndefinedBehaviorSanitizer, like abi_args_bwd_support.cpp: built by
// `make -C nwhead_amd/csrc sanitize_bwd_values_bank` from the library's own sources with --cuda-host-only against
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
    const size_t need = nw_bwd_values_bank_support_workspace_bytes(8, 1000, 64, 32, 0);
    EXPECT(need > 0, 1);
    // forced query chunks size the partial tiles; one chunk holds nothing of size N x d, and nothing of size B x N or
    // N x T at the shapes the design quotes
    EXPECT(nw_bwd_values_bank_support_workspace_bytes(200, 1000, 64, 64, 3) >
               nw_bwd_values_bank_support_workspace_bytes(200, 1000, 64, 64, 1) + (size_t)2 * 1000 * 64 * 4, 1);
    EXPECT(nw_bwd_values_bank_support_workspace_bytes(200, 1000, 64, 64, 1) < (size_t)1000 * 64 * 4, 1);
    EXPECT(nw_bwd_values_bank_support_workspace_bytes(200, 1000, 64, 64, 1) == nw_bwd_values_bank_support_workspace_bytes(200, 1000, 64, 16384, 1), 1);
    EXPECT(nw_bwd_values_bank_support_workspace_bytes(256, 50000, 512, 512, 0) < (size_t)256 * 50000 * 4, 1);
    EXPECT(nw_bwd_values_bank_support_workspace_bytes(256, 400000, 256, 32, 0) < (size_t)256 * 400000 * 4, 1);
    // outside the regime, or nothing to do: 0
    EXPECT(nw_bwd_values_bank_support_workspace_bytes(0, 1000, 64, 32, 0), 0);
    EXPECT(nw_bwd_values_bank_support_workspace_bytes(-1, 1000, 64, 32, 0), 0);
    EXPECT(nw_bwd_values_bank_support_workspace_bytes(8, 25, 64, 32, 0), 0);
    EXPECT(nw_bwd_values_bank_support_workspace_bytes(8, 1000, 100, 32, 0), 0);
    EXPECT(nw_bwd_values_bank_support_workspace_bytes(8, 1000, 16, 32, 0), 0);
    EXPECT(nw_bwd_values_bank_support_workspace_bytes(8, 1000, 64, 0, 0), 0);
    EXPECT(nw_bwd_values_bank_support_workspace_bytes(8, 1000, 64, 5, 0), 0);
    EXPECT(nw_bwd_values_bank_support_workspace_bytes(8, 1000, 64, 16384 + 32, 0), 0);
    EXPECT(nw_bwd_values_bank_support_workspace_bytes(8, 1000, 64, 32, -1), 0);
    EXPECT(nw_bwd_values_bank_support_workspace_bytes(8, 1000, 64, 16384, 0) > 0, 1);

#define SUP(q, s, ssplit, vsplit, vscale, a, lo, hi, ex, lse, out, gout, gs, wsp, wsb, B, N, d, T, kind, chunks) \
    nw_bwd_values_bank_support_f32(q, s, ssplit, F, F, vsplit, vscale, a, lo, hi, ex, lse, out, gout, gs, wsp, wsb, B, N, d, T, kind, nullptr, chunks, nullptr)
    // the window is both arrays or neither
    EXPECT(SUP(F, F, F, F, F, F, nullptr, HI, 0, F, F, F, F, ws, sizeof ws, 8, 1000, 64, 32, E, 0), NW_ERR_INVALID_ARG);
    EXPECT(SUP(F, F, F, F, F, F, LO, nullptr, 1, F, F, F, F, ws, sizeof ws, 8, 1000, 64, 32, E, 0), NW_ERR_INVALID_ARG);
    for (int weighted = 0; weighted < 2; ++weighted) {
        const float* a = weighted ? F : nullptr;
        for (int windowed = 0; windowed < 2; ++windowed) {
            const int32_t *lo = windowed ? LO : nullptr, *hi = windowed ? HI : nullptr;
            for (int ex = 0; ex < 2; ++ex) {
                // negative sizes, null operands, clip without its scale
                EXPECT(SUP(F, F, F, F, F, a, lo, hi, ex, F, F, F, F, ws, sizeof ws, -1, 1000, 64, 32, E, 0), NW_ERR_INVALID_ARG);
                EXPECT(SUP(F, F, F, F, F, a, lo, hi, ex, F, F, F, F, ws, sizeof ws, 8, -1, 64, 32, E, 0), NW_ERR_INVALID_ARG);
                EXPECT(SUP(F, F, F, F, F, a, lo, hi, ex, F, F, F, F, ws, sizeof ws, 8, 1000, -64, 32, E, 0), NW_ERR_INVALID_ARG);
                EXPECT(SUP(F, F, F, F, F, a, lo, hi, ex, F, F, F, F, ws, sizeof ws, 8, 1000, 64, -32, E, 0), NW_ERR_INVALID_ARG);
                EXPECT(SUP(F, F, F, F, F, a, lo, hi, ex, F, F, F, F, ws, sizeof ws, 8, 1000, 64, 32, E, -1), NW_ERR_INVALID_ARG);
                EXPECT(SUP(nullptr, F, F, F, F, a, lo, hi, ex, F, F, F, F, ws, sizeof ws, 8, 1000, 64, 32, E, 0), NW_ERR_INVALID_ARG);
                EXPECT(SUP(F, nullptr, F, F, F, a, lo, hi, ex, F, F, F, F, ws, sizeof ws, 8, 1000, 64, 32, E, 0), NW_ERR_INVALID_ARG);
                EXPECT(SUP(F, F, nullptr, F, F, a, lo, hi, ex, F, F, F, F, ws, sizeof ws, 8, 1000, 64, 32, E, 0), NW_ERR_INVALID_ARG);
                EXPECT(SUP(F, F, F, nullptr, F, a, lo, hi, ex, F, F, F, F, ws, sizeof ws, 8, 1000, 64, 32, E, 0), NW_ERR_INVALID_ARG);
                EXPECT(SUP(F, F, F, F, nullptr, a, lo, hi, ex, F, F, F, F, ws, sizeof ws, 8, 1000, 64, 32, E, 0), NW_ERR_INVALID_ARG);
                EXPECT(SUP(F, F, F, F, F, a, lo, hi, ex, nullptr, F, F, F, ws, sizeof ws, 8, 1000, 64, 32, E, 0), NW_ERR_INVALID_ARG);
                EXPECT(SUP(F, F, F, F, F, a, lo, hi, ex, F, nullptr, F, F, ws, sizeof ws, 8, 1000, 64, 32, E, 0), NW_ERR_INVALID_ARG);
                EXPECT(SUP(F, F, F, F, F, a, lo, hi, ex, F, F, nullptr, F, ws, sizeof ws, 8, 1000, 64, 32, E, 0), NW_ERR_INVALID_ARG);
                EXPECT(SUP(F, F, F, F, F, a, lo, hi, ex, F, F, F, nullptr, ws, sizeof ws, 8, 1000, 64, 32, E, 0), NW_ERR_INVALID_ARG);
                EXPECT(SUP(F, F, F, F, F, a, lo, hi, ex, F, F, F, F, ws, sizeof ws, 8, 1000, 64, 32, NW_SCORE_CLIP, 0), NW_ERR_INVALID_ARG);
                // outside the regime
                EXPECT(SUP(F, F, F, F, F, a, lo, hi, ex, F, F, F, F, ws, sizeof ws, 8, 1000, 64, 32, 99, 0), NW_ERR_UNSUPPORTED);
                EXPECT(SUP(F, F, F, F, F, a, lo, hi, ex, F, F, F, F, ws, sizeof ws, 8, 1000, 100, 32, E, 0), NW_ERR_UNSUPPORTED);
                EXPECT(SUP(F, F, F, F, F, a, lo, hi, ex, F, F, F, F, ws, sizeof ws, 8, 1000, 16, 32, E, 0), NW_ERR_UNSUPPORTED);
                EXPECT(SUP(F, F, F, F, F, a, lo, hi, ex, F, F, F, F, ws, sizeof ws, 8, 25, 64, 32, E, 0), NW_ERR_UNSUPPORTED);
                EXPECT(SUP(F, F, F, F, F, a, lo, hi, ex, F, F, F, F, ws, sizeof ws, 8, 1000, 64, 0, E, 0), NW_ERR_UNSUPPORTED);
                EXPECT(SUP(F, F, F, F, F, a, lo, hi, ex, F, F, F, F, ws, sizeof ws, 8, 1000, 64, 5, E, 0), NW_ERR_UNSUPPORTED);
                EXPECT(SUP(F, F, F, F, F, a, lo, hi, ex, F, F, F, F, ws, sizeof ws, 8, 1000, 64, 16384 + 32, E, 0), NW_ERR_UNSUPPORTED);
                EXPECT(SUP(F + 1, F, F, F, F, a, lo, hi, ex, F, F, F, F, ws, sizeof ws, 8, 1000, 64, 32, E, 0), NW_ERR_UNSUPPORTED);
                EXPECT(SUP(F, F + 1, F, F, F, a, lo, hi, ex, F, F, F, F, ws, sizeof ws, 8, 1000, 64, 32, E, 0), NW_ERR_UNSUPPORTED);
                EXPECT(SUP(F, F, F + 1, F, F, a, lo, hi, ex, F, F, F, F, ws, sizeof ws, 8, 1000, 64, 32, E, 0), NW_ERR_UNSUPPORTED);
                EXPECT(SUP(F, F, F, F + 1, F, a, lo, hi, ex, F, F, F, F, ws, sizeof ws, 8, 1000, 64, 32, E, 0), NW_ERR_UNSUPPORTED);
                EXPECT(SUP(F, F, F, F, F, a, lo, hi, ex, F, F, F + 1, F, ws, sizeof ws, 8, 1000, 64, 32, E, 0), NW_ERR_UNSUPPORTED);
                EXPECT(SUP(F, F, F, F, F, a, lo, hi, ex, F, F, F, F + 1, ws, sizeof ws, 8, 1000, 64, 32, E, 0), NW_ERR_UNSUPPORTED);
                if (a) EXPECT(SUP(F, F, F, F, F, F + 1, lo, hi, ex, F, F, F, F, ws, sizeof ws, 8, 1000, 64, 32, E, 0), NW_ERR_UNSUPPORTED);
                // the workspace
                EXPECT(SUP(F, F, F, F, F, a, lo, hi, ex, F, F, F, F, ws, sizeof ws, 8, 1000, 64, 32, E, 0), NW_ERR_WORKSPACE);
                EXPECT(SUP(F, F, F, F, F, a, lo, hi, ex, F, F, F, F, nullptr, need, 8, 1000, 64, 32, E, 0), NW_ERR_WORKSPACE);
                EXPECT(SUP(F, F, F, F, F, a, lo, hi, ex, F, F, F, F, ws, need - 1, 8, 1000, 64, 32, E, 0), NW_ERR_WORKSPACE);
                EXPECT(SUP(F, F, F, F, F, a, lo, hi, ex, F, F, F, F, ws + 4, need, 8, 1000, 64, 32, E, 0), NW_ERR_UNSUPPORTED);
                // B == 0: NW_OK, nothing is read, nothing is launched, nothing is written
                EXPECT(SUP(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, lo, hi, ex, nullptr, nullptr, nullptr, nullptr, nullptr, 0,
                           0, 1000, 64, 32, E, 0), NW_OK);
            }
        }
    }
    std::printf(failures ? "abi_args_bwd_values_bank: %d FAILED\n"
                         : "abi_args_bwd_values_bank: all argument checks refused as documented\n",
                failures);
    return failures ? 1 : 0;
}
