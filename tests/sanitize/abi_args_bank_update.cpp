// Host-only exercise of nw_bank_update_rows_f32 (include/nwhead_hip.h) under AddressSanitizer + UndefinedBehaviorSanitizer,
// like abi_args_fwd_window.cpp: built by `make -C nwhead_amd/csrc sanitize_bank_update` from the library's own sources with
// --cuda-host-only against hip_stubs.cpp.  Every call here must be refused BEFORE anything is launched (or, with R == 0 or
// N == 0, answered), with the documented status and without a sanitizer report.  The rows follow the order of the status
// list in the header: each call is well formed in everything the earlier rows check.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>
#include "../../include/nwhead_hip.h"
#include "expect.h"

int main() {
    alignas(16) static float F[4096];
    alignas(16) static uint16_t H[4096];
    std::vector<int64_t> rows(64, 0);
    const int64_t* RW = rows.data();
    float* const Z = nullptr;
    const float inf = INFINITY, nan = NAN;
    // (x, rows, R, dx, momentum, s_rows, s_user, s_norm2, s_split, s_scale, s_f16, f16_scale, f16_norm2, N, d, stream)
    // ---- negative sizes
    EXPECT(nw_bank_update_rows_f32(F, RW, -1, 64, 0.f, F, Z, F, F, F, nullptr, Z, Z, 64, 64, nullptr), NW_ERR_INVALID_ARG);
    EXPECT(nw_bank_update_rows_f32(F, RW, 8, 64, 0.f, F, Z, F, F, F, nullptr, Z, Z, -64, 64, nullptr), NW_ERR_INVALID_ARG);
    EXPECT(nw_bank_update_rows_f32(F, RW, 8, 64, 0.f, F, Z, F, F, F, nullptr, Z, Z, 64, -64, nullptr), NW_ERR_INVALID_ARG);
    // ---- dx outside [1, d], also with nothing to do
    EXPECT(nw_bank_update_rows_f32(F, RW, 8, 0, 0.f, F, Z, F, F, F, nullptr, Z, Z, 64, 64, nullptr), NW_ERR_INVALID_ARG);
    EXPECT(nw_bank_update_rows_f32(F, RW, 8, -4, 0.f, F, Z, F, F, F, nullptr, Z, Z, 64, 64, nullptr), NW_ERR_INVALID_ARG);
    EXPECT(nw_bank_update_rows_f32(F, RW, 8, 65, 0.f, F, Z, F, F, F, nullptr, Z, Z, 64, 64, nullptr), NW_ERR_INVALID_ARG);
    EXPECT(nw_bank_update_rows_f32(F, RW, 0, 65, 0.f, F, Z, F, F, F, nullptr, Z, Z, 64, 64, nullptr), NW_ERR_INVALID_ARG);
    EXPECT(nw_bank_update_rows_f32(F, RW, 8, 1, 0.f, F, Z, F, F, F, nullptr, Z, Z, 64, 0, nullptr), NW_ERR_INVALID_ARG);
    // ---- momentum not finite or outside [0, 1), also with nothing to do
    const float bad_m[] = {-0.5f, 1.f, 1.5f, inf, -inf, nan};
    for (float m : bad_m) {
        EXPECT(nw_bank_update_rows_f32(F, RW, 8, 64, m, F, Z, F, F, F, nullptr, Z, Z, 64, 64, nullptr), NW_ERR_INVALID_ARG);
        EXPECT(nw_bank_update_rows_f32(F, RW, 0, 64, m, F, Z, F, F, F, nullptr, Z, Z, 64, 64, nullptr), NW_ERR_INVALID_ARG);
    }
    // ---- R == 0 or N == 0: NW_OK, nothing is read, nothing is launched
    EXPECT(nw_bank_update_rows_f32(nullptr, nullptr, 0, 64, 0.5f, Z, Z, Z, Z, Z, nullptr, Z, Z, 64, 64, nullptr), NW_OK);
    EXPECT(nw_bank_update_rows_f32(nullptr, nullptr, 8, 64, 0.f, Z, Z, Z, Z, Z, nullptr, Z, Z, 0, 64, nullptr), NW_OK);
    EXPECT(nw_bank_update_rows_f32(F, RW, 0, 20, 0.f, F + 1, Z, F, F, Z, nullptr, Z, Z, 64, 20, nullptr), NW_OK);
    // ---- null x, rows, s_rows, s_norm2
    EXPECT(nw_bank_update_rows_f32(nullptr, RW, 8, 64, 0.f, F, Z, F, F, F, nullptr, Z, Z, 64, 64, nullptr), NW_ERR_INVALID_ARG);
    EXPECT(nw_bank_update_rows_f32(F, nullptr, 8, 64, 0.f, F, Z, F, F, F, nullptr, Z, Z, 64, 64, nullptr), NW_ERR_INVALID_ARG);
    EXPECT(nw_bank_update_rows_f32(F, RW, 8, 64, 0.f, Z, Z, F, F, F, nullptr, Z, Z, 64, 64, nullptr), NW_ERR_INVALID_ARG);
    EXPECT(nw_bank_update_rows_f32(F, RW, 8, 64, 0.f, F, Z, Z, F, F, nullptr, Z, Z, 64, 64, nullptr), NW_ERR_INVALID_ARG);
    // ---- a form group given in part
    EXPECT(nw_bank_update_rows_f32(F, RW, 8, 64, 0.f, F, Z, F, F, Z, nullptr, Z, Z, 64, 64, nullptr), NW_ERR_INVALID_ARG);
    EXPECT(nw_bank_update_rows_f32(F, RW, 8, 64, 0.f, F, Z, F, Z, F, nullptr, Z, Z, 64, 64, nullptr), NW_ERR_INVALID_ARG);
    EXPECT(nw_bank_update_rows_f32(F, RW, 8, 192, 0.f, F, Z, F, Z, Z, H, F, Z, 8, 192, nullptr), NW_ERR_INVALID_ARG);
    EXPECT(nw_bank_update_rows_f32(F, RW, 8, 192, 0.f, F, Z, F, Z, Z, H, Z, F, 8, 192, nullptr), NW_ERR_INVALID_ARG);
    EXPECT(nw_bank_update_rows_f32(F, RW, 8, 192, 0.f, F, Z, F, Z, Z, nullptr, F, F, 8, 192, nullptr), NW_ERR_INVALID_ARG);
    EXPECT(nw_bank_update_rows_f32(F, RW, 8, 192, 0.f, F, Z, F, F, F, H, F, Z, 8, 192, nullptr), NW_ERR_INVALID_ARG);
    // ---- s_rows, s_split or s_f16 not 16-byte aligned (x may be anything)
    EXPECT(nw_bank_update_rows_f32(F, RW, 8, 64, 0.f, F + 1, Z, F, F, F, nullptr, Z, Z, 64, 64, nullptr), NW_ERR_INVALID_ARG);
    EXPECT(nw_bank_update_rows_f32(F, RW, 8, 64, 0.f, F, Z, F, F + 2, F, nullptr, Z, Z, 64, 64, nullptr), NW_ERR_INVALID_ARG);
    EXPECT(nw_bank_update_rows_f32(F, RW, 8, 192, 0.f, F, Z, F, Z, Z, H + 4, F, F, 8, 192, nullptr), NW_ERR_INVALID_ARG);
    // ---- neither form group: a norms-only bank
    EXPECT(nw_bank_update_rows_f32(F, RW, 8, 64, 0.f, F, Z, F, Z, Z, nullptr, Z, Z, 64, 64, nullptr), NW_ERR_UNSUPPORTED);
    EXPECT(nw_bank_update_rows_f32(F + 1, RW, 8, 20, 0.5f, F, Z, F, Z, Z, nullptr, Z, Z, 64, 20, nullptr), NW_ERR_UNSUPPORTED);
    // ---- the split group with d % 32 != 0
    EXPECT(nw_bank_update_rows_f32(F, RW, 8, 48, 0.f, F, Z, F, F, F, nullptr, Z, Z, 64, 48, nullptr), NW_ERR_UNSUPPORTED);
    EXPECT(nw_bank_update_rows_f32(F, RW, 8, 20, 0.f, F, F, F, F, F, nullptr, Z, Z, 64, 100, nullptr), NW_ERR_UNSUPPORTED);
    // ---- the fp16 group with d % 64 != 0 or d < 192
    EXPECT(nw_bank_update_rows_f32(F, RW, 8, 224, 0.f, F, Z, F, Z, Z, H, F, F, 8, 224, nullptr), NW_ERR_UNSUPPORTED);
    EXPECT(nw_bank_update_rows_f32(F, RW, 8, 128, 0.f, F, Z, F, Z, Z, H, F, F, 8, 128, nullptr), NW_ERR_UNSUPPORTED);
    EXPECT(nw_bank_update_rows_f32(F, RW, 8, 64, 0.f, F, Z, F, Z, Z, H, F, F, 8, 64, nullptr), NW_ERR_UNSUPPORTED);
    EXPECT(nw_bank_update_rows_f32(F, RW, 8, 96, 0.f, F, Z, F, F, F, H, F, F, 8, 96, nullptr), NW_ERR_UNSUPPORTED);      // both groups
    // ---- more items than a wave scans
    EXPECT(nw_bank_update_rows_f32(F, RW, 16385, 64, 0.f, F, Z, F, F, F, nullptr, Z, Z, 64, 64, nullptr), NW_ERR_UNSUPPORTED);
    EXPECT(nw_bank_update_rows_f32(F, RW, 16385, 192, 0.9f, F, Z, F, Z, Z, H, F, F, 8, 192, nullptr), NW_ERR_UNSUPPORTED);
    std::printf(failures ? "abi_args_bank_update: %d FAILED\n" : "abi_args_bank_update: all argument checks refused as documented\n",
                failures);
    return failures ? 1 : 0;
}
