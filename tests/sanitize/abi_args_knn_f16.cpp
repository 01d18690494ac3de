// Host-only exercise of nw_knn_f16 / nw_knn_f16_workspace_bytes (include/nwhead_hip.h) under AddressSanitizer +
// UndefinedBehaviorSanitizer, like abi_args.cpp: built by `make -C nwhead_amd/csrc sanitize_knn_f16` from the library's
// own sources with --cuda-host-only against hip_stubs.cpp.  Every call here is a pure host computation or must be refused
// BEFORE anything is launched, with the documented status and without a sanitizer report.
#include <cstdint>
#include <cstdio>
#include <vector>
#include "../../include/nwhead_hip.h"
#include "expect.h"

static size_t cand_slots(int64_t k) { return (size_t)(((k < 128 ? k : 128) + 3) & ~(int64_t)3); }

int main() {
    alignas(16) static float F[4096];
    alignas(16) static char ws[256];
    std::vector<int64_t> idx(64, 0);
    int64_t* I = idx.data();
    const void* H = F;   // stands for the fp16 rows: never read on the host
    const int E = NW_SCORE_EUCLIDEAN;
    // ---- sizes: pure host arithmetic
    EXPECT(nw_knn_f16_workspace_bytes(0, 1000, 192, 10), 0);
    EXPECT(nw_knn_f16_workspace_bytes(-1, 1000, 192, 10), 0);
    EXPECT(nw_knn_f16_workspace_bytes(8, 1000, 100, 10), 0);     // width outside the half form
    EXPECT(nw_knn_f16_workspace_bytes(8, 1000, 128, 10), 0);     // fewer than three 64-k stages
    EXPECT(nw_knn_f16_workspace_bytes(8, 1000, 192, 33), 0);
    EXPECT(nw_knn_f16_workspace_bytes(8, 1000, 192, 0), 0);
    EXPECT(nw_knn_f16_workspace_bytes(8, 25, 192, 5), 0);        // N <= 25: no tile kernel
    EXPECT(nw_knn_f16_workspace_bytes(8, 30, 192, 31), 0);       // k > N
    EXPECT(nw_knn_f16_workspace_bytes((int64_t)1 << 30, 1000, 192, 10), 0);
    const size_t need = nw_knn_f16_workspace_bytes(8, 1000, 192, 10);
    EXPECT(need >= 2 * 4 * (size_t)8 * 8 * cand_slots(10) + (size_t)8 * 192 * 2 + 2 * 8 * 4, 1);
    EXPECT(nw_knn_f16_workspace_bytes(9, 1000, 192, 10) >= need, 1);
    EXPECT(nw_knn_f16_workspace_bytes(8, 1025, 192, 10) >= need, 1);
    EXPECT(nw_knn_f16_workspace_bytes(8, 1000, 192, 13) >= need, 1);
    // a large shape: no overflow on the way (256 x 400000 x 256, k = 32: 3125 tiles of 32 slots, twice 4 bytes)
    EXPECT(nw_knn_f16_workspace_bytes(256, 400000, 256, 32) >= (size_t)2 * 4 * 256 * 3125 * 32, 1);
    EXPECT(nw_knn_f16_workspace_bytes(((int64_t)1 << 30) - 1, ((int64_t)1 << 30) - 1, 192, 32) > ((size_t)1 << 60), 1);
    // ---- the search: refused before any launch
    EXPECT(nw_knn_f16(F, H, F, F, I, nullptr, ws, sizeof ws, -1, 1000, 192, 10, E, nullptr, nullptr, nullptr), NW_ERR_INVALID_ARG);
    EXPECT(nw_knn_f16(F, H, F, F, I, nullptr, ws, sizeof ws, 8, -1, 192, 10, E, nullptr, nullptr, nullptr), NW_ERR_INVALID_ARG);
    EXPECT(nw_knn_f16(F, H, F, F, I, nullptr, ws, sizeof ws, 8, 1000, -192, 10, E, nullptr, nullptr, nullptr), NW_ERR_INVALID_ARG);
    EXPECT(nw_knn_f16(F, H, F, F, I, nullptr, ws, sizeof ws, 8, 1000, 192, 10, 99, nullptr, nullptr, nullptr), NW_ERR_UNSUPPORTED);
    EXPECT(nw_knn_f16(nullptr, H, F, F, I, nullptr, ws, sizeof ws, 8, 1000, 192, 10, E, nullptr, nullptr, nullptr), NW_ERR_INVALID_ARG);
    EXPECT(nw_knn_f16(F, nullptr, F, F, I, nullptr, ws, sizeof ws, 8, 1000, 192, 10, E, nullptr, nullptr, nullptr), NW_ERR_INVALID_ARG);
    EXPECT(nw_knn_f16(F, H, nullptr, F, I, nullptr, ws, sizeof ws, 8, 1000, 192, 10, E, nullptr, nullptr, nullptr), NW_ERR_INVALID_ARG);
    EXPECT(nw_knn_f16(F, H, F, nullptr, I, nullptr, ws, sizeof ws, 8, 1000, 192, 10, E, nullptr, nullptr, nullptr), NW_ERR_INVALID_ARG);
    EXPECT(nw_knn_f16(F, H, F, F, nullptr, nullptr, ws, sizeof ws, 8, 1000, 192, 10, E, nullptr, nullptr, nullptr), NW_ERR_INVALID_ARG);
    EXPECT(nw_knn_f16(F, H, F, F, I, nullptr, ws, sizeof ws, 8, 1000, 192, 10, NW_SCORE_CLIP, nullptr, nullptr, nullptr),
           NW_ERR_INVALID_ARG);                                                                     // clip without logit_scale
    EXPECT(nw_knn_f16(F + 1, H, F, F, I, nullptr, ws, sizeof ws, 8, 1000, 192, 10, E, nullptr, nullptr, nullptr), NW_ERR_INVALID_ARG);
    EXPECT(nw_knn_f16(F, F + 1, F, F, I, nullptr, ws, sizeof ws, 8, 1000, 192, 10, E, nullptr, nullptr, nullptr), NW_ERR_INVALID_ARG);
    EXPECT(nw_knn_f16(F, H, F, F, I, nullptr, ws + 4, sizeof ws - 4, 8, 1000, 192, 10, E, nullptr, nullptr, nullptr), NW_ERR_INVALID_ARG);
    EXPECT(nw_knn_f16(F, H, F, F, I, nullptr, ws, sizeof ws, 8, 1000, 100, 10, E, nullptr, nullptr, nullptr), NW_ERR_UNSUPPORTED);
    EXPECT(nw_knn_f16(F, H, F, F, I, nullptr, ws, sizeof ws, 8, 1000, 128, 10, E, nullptr, nullptr, nullptr), NW_ERR_UNSUPPORTED);
    EXPECT(nw_knn_f16(F, H, F, F, I, nullptr, ws, sizeof ws, 8, 1000, 192, 33, E, nullptr, nullptr, nullptr), NW_ERR_UNSUPPORTED);
    EXPECT(nw_knn_f16(F, H, F, F, I, nullptr, ws, sizeof ws, 8, 1000, 192, 0, E, nullptr, nullptr, nullptr), NW_ERR_UNSUPPORTED);
    EXPECT(nw_knn_f16(F, H, F, F, I, nullptr, ws, sizeof ws, 8, 20, 192, 5, E, nullptr, nullptr, nullptr), NW_ERR_UNSUPPORTED);
    EXPECT(nw_knn_f16(F, H, F, F, I, nullptr, ws, sizeof ws, 8, 30, 192, 31, E, nullptr, nullptr, nullptr), NW_ERR_UNSUPPORTED);
    EXPECT(nw_knn_f16(F, H, F, F, I, nullptr, ws, sizeof ws, 8, 1000, 192, 10, E, nullptr, nullptr, nullptr), NW_ERR_WORKSPACE);
    EXPECT(nw_knn_f16(F, H, F, F, I, nullptr, nullptr, 0, 8, 1000, 192, 10, E, nullptr, nullptr, nullptr), NW_ERR_WORKSPACE);
    EXPECT(nw_knn_f16(F, H, F, F, I, nullptr, ws, need - 1, 8, 1000, 192, 10, E, nullptr, nullptr, nullptr), NW_ERR_WORKSPACE);
    // zero sizes: B == 0 is NW_OK whatever else is passed (nothing is read, nothing is launched)
    EXPECT(nw_knn_f16(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, 1000, 192, 10, E, nullptr, nullptr,
                      nullptr), NW_OK);
    EXPECT(nw_knn_f16(F, H, F, F, I, nullptr, nullptr, 0, 0, 1000, 192, 10, E, nullptr, nullptr, nullptr), NW_OK);
    EXPECT(nw_knn_f16(F, H, F, F, I, nullptr, ws, sizeof ws, 8, 0, 192, 10, E, nullptr, nullptr, nullptr), NW_ERR_UNSUPPORTED);
    // options: a full struct, and one too short to hold persistent_wgs (read as no options); neither changes a refusal
    nw_fwd_opts o = {};
    o.struct_size = sizeof o;
    o.persistent_wgs = 8;
    EXPECT(nw_knn_f16(F, H, F, F, I, nullptr, ws, sizeof ws, 8, 1000, 192, 10, E, nullptr, &o, nullptr), NW_ERR_WORKSPACE);
    EXPECT(nw_knn_f16(F, H, F, F, I, nullptr, ws, sizeof ws, 8, 1000, 100, 10, E, nullptr, &o, nullptr), NW_ERR_UNSUPPORTED);
    uint32_t tiny = sizeof tiny;   // struct_size alone
    EXPECT(nw_knn_f16(F, H, F, F, I, nullptr, ws, sizeof ws, 8, 1000, 192, 10, E, nullptr,
                      reinterpret_cast<const nw_fwd_opts*>(&tiny), nullptr), NW_ERR_WORKSPACE);
    std::printf(failures ? "abi_args_knn_f16: %d FAILED\n" : "abi_args_knn_f16: all argument checks refused as documented\n",
                failures);
    return failures ? 1 : 0;
}
