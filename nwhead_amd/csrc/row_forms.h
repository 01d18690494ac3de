// The per-row arithmetic of the prepared forms of a bank row (split.hip, backward.hip): ONE copy, shared by the kernels that
// prepare whole matrices (nw_split_rows_f16x2, nw_pack_rows_f16, nw_row_norm2_f32) and the one that refreshes single rows
// of a prepared bank in place (nw_bank_update_rows_f32), which has to leave the bits the others would have written.
// A wave holds a row as 4-float chunks: chunk c of lane (c % 64), in ascending c per lane.
#pragma once
#include "nw_internal.h"

namespace nw {

typedef _Float16 half4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float row_amax4(float m, const float4 v) {
    return fmaxf(fmaxf(m, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
}

// one chunk's share of the split form's statistics: largest magnitude and sum of squares of the ORIGINAL values
__device__ __forceinline__ void row_split_accum(float& mx, float& n2, const float4 v) {
    mx = fmaxf(fmaxf(mx, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
    n2 += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
}

// e with mx * 2^e in [2^13, 2^14) for the row's largest magnitude mx (already reduced over the wave); 0 for a row of
// zeros or one that holds an infinity
__device__ __forceinline__ int row_scale_exponent(float mx) {
    int e = 0;
    if (mx > 0.f && mx < INFINITY) {
        frexpf(mx, &e);   // mx = f * 2^e, f in [0.5, 1)
        e = 14 - e;       // mx * 2^e in [2^13, 2^14)
        if (e > 126) e = 126;  // a row of subnormal magnitudes (max < 2^-112): 2^e must stay finite and 2^-e normal
    }
    return e;
}

// chunk c (4 floats) of the row -> halves 4*(c % 8) .. +3 of the 32-k chunk c / 8: [32 x h | 32 x l] (tile_f16.h)
__device__ __forceinline__ void row_split_emit(_Float16* dst, int64_t c, const float4 v, float up, unsigned lmask) {
    const float sv[4] = {v.x * up, v.y * up, v.z * up, v.w * up};
    half4 h, l;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        h[k] = (_Float16)sv[k];
        l[k] = (_Float16)(sv[k] - (float)h[k]);
    }
    if (lmask != 0xffffu) {  // diagnostic (NW_SPLIT_LBITS): fewer significant bits in the low halves
        typedef unsigned short us4 __attribute__((ext_vector_type(4)));
        us4 b = __builtin_bit_cast(us4, l);
        b &= (unsigned short)lmask;
        l = __builtin_bit_cast(half4, b);
    }
    const int64_t chunk = c >> 3, within = (c & 7) * 4;
    *reinterpret_cast<half4*>(dst + chunk * 64 + within) = h;
    *reinterpret_cast<half4*>(dst + chunk * 64 + 32 + within) = l;
}

// chunk c of the row -> its four fp16 values in the dense fp16 row; n2 gathers the squares of the ROUNDED values
__device__ __forceinline__ void row_pack_emit(half4* dst, int64_t c, const float4 v, float up, float down, float& n2) {
    const float sv[4] = {v.x * up, v.y * up, v.z * up, v.w * up};
    half4 h;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        h[k] = (_Float16)sv[k];
        const float back = (float)h[k] * down;
        n2 = __builtin_fmaf(back, back, n2);
    }
    dst[c] = h;
}

// a lane's share of the plain squared norm (nw_row_norm2_f32): elements lane, lane + 64, ... of the row, in that order
template <typename At>
__device__ __forceinline__ float row_norm2_lane(At at, int64_t d, int lane) {
    float a = 0.f;
    for (int64_t k = lane; k < d; k += 64) {
        const float v = at(k);
        a += v * v;
    }
    return a;
}

}  // namespace nw
