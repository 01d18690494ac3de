// split.hip -- fp32 rows -> "split rows" for the fp16 matrix cores (gfx950 / MI355X only).
//
// For every row: e = power-of-two exponent that brings the row's largest magnitude into
// [2^13, 2^14); every 32-float chunk of the scaled row becomes [32 x h | 32 x l] (fp16), h = fp16(x),
// l = fp16(x - h): same bytes, same row stride as the fp32 original (format: tile_f16.h).  Also written:
// scale[r] = 2^-e (what undoes the scaling of a dot product) and norm2[r] = sum_k x_k^2 in fp32 of the
// ORIGINAL values (the pow(2).sum(-1) half of torch.cdist's matmul form).
// One wave per row; HBM-bound streaming (8*d bytes per row).
#include "nw_internal.h"
#include "row_forms.h"
#include <type_traits>
#include <cstdlib>

namespace nw {
namespace {

__global__ __launch_bounds__(256) void nw_split_rows_kernel(const float* __restrict__ x,
                                                             float* __restrict__ out,
                                                             float* __restrict__ scale,
                                                             float* __restrict__ norm2, int64_t rows,
                                                             int64_t d, unsigned lmask) {
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (r >= rows) return;
    const float4* src = reinterpret_cast<const float4*>(x + r * d);
    const int64_t n4 = d / 4;
    // rows up to 64*4*KEEP floats stay in registers: ONE round of loads (the query batch is split
    // inside every forward call, where this kernel is pure latency)
    constexpr int KEEP = 8;
    const bool in_regs = n4 <= 64 * KEEP;
    float4 keep[KEEP];
    float mx = 0.f, n2 = 0.f;
    if (in_regs) {
#pragma unroll
        for (int u = 0; u < KEEP; ++u) {
            const int64_t c = lane + 64 * u;
            keep[u] = (c < n4) ? src[c] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int u = 0; u < KEEP; ++u) row_split_accum(mx, n2, keep[u]);
    } else {
        for (int64_t c = lane; c < n4; c += 64) row_split_accum(mx, n2, src[c]);
    }
    mx = wave_max(mx);
    n2 = wave_sum(n2);
    const int e = row_scale_exponent(mx);
    const float up = ldexpf(1.f, e);
    if (lane == 0) {
        scale[r] = ldexpf(1.f, -e);
        norm2[r] = n2;
    }
    _Float16* dst = reinterpret_cast<_Float16*>(out + r * d);
    auto emit = [&](int64_t c, const float4 v) { row_split_emit(dst, c, v, up, lmask); };
    if (in_regs) {
#pragma unroll
        for (int u = 0; u < KEEP; ++u) {
            const int64_t c = lane + 64 * u;
            if (c < n4) emit(c, keep[u]);
        }
    } else {
        for (int64_t c = lane; c < n4; c += 64) emit(c, src[c]);
    }
}

}  // namespace

// The mask of the low halves under the "split_lbits" knob (0xffff: all bits, the default).
static unsigned split_lmask() {
    // Mantissa bits kept in the low halves (default 10 = all: the split is exact to 22 bits).  The tile kernel's pace
    // follows the operands' bit activity: K3 launch 583 us at 10 bits, 572 at 6, 563 at 3, 556 at 0 (max error vs fp64
    // 0.9 / 1.1 / 3.7 / 24 e-6).  Not taken: the large-norm, small-distance cases (golden G8) need the bits.  (Diagnostic
    // knob "split_lbits".)
    const int kb = knob(KNOB_SPLIT_LBITS);
    const int keep = kb == KNOB_UNSET ? 10 : kb;
    return keep >= 10 ? 0xffffu : (0xffffu << (10 - (keep < 0 ? 0 : keep))) & 0xffffu;
}

int launch_split_rows(const float* x, float* out, float* scale, float* norm2, int64_t rows, int64_t d,
                      hipStream_t st) {
    if (rows <= 0) return NW_OK;
    if ((rows + 3) / 4 > 0x7fffffffLL) return NW_ERR_INVALID_ARG;
    hipLaunchKernelGGL(nw_split_rows_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, x, out, scale,
                       norm2, rows, d, split_lmask());
    NW_CHECK_LAUNCH();
    return NW_OK;
}

}  // namespace nw

extern "C" int nw_split_rows_f16x2(const float* x, float* out_split, float* row_scale, float* row_norm2,
                                   int64_t rows, int64_t d, void* stream) {
    if (rows < 0 || d < 0) return NW_ERR_INVALID_ARG;
    if (d % 32 != 0) return NW_ERR_UNSUPPORTED;
    if (rows == 0) return NW_OK;
    if (!x || !out_split || !row_scale || !row_norm2) return NW_ERR_INVALID_ARG;
    if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(out_split)) & 15) return NW_ERR_INVALID_ARG;
    return nw::launch_split_rows(x, out_split, row_scale, row_norm2, rows, d, static_cast<hipStream_t>(stream));
}

// ------------------------------------------------------------------------------------------------------------------
// fp32 rows -> plain fp16 rows (nw_pack_rows_f16): the operand of the half-precision head (nw_fwd_opts.operand_form = 1).
// The scale rule of nw_split_rows_kernel, but only h = fp16(x * 2^e) is kept, as a dense (rows, d) fp16 matrix, and
// norm2[r] = sum_k (h_k * 2^-e)^2: the norms of the ROUNDED rows, so that the head of these operands is the exact head of
// the rounded features.  One wave per row; 4*d bytes in, 2*d out.
namespace nw {
namespace {

__global__ __launch_bounds__(256) void nw_pack_rows_f16_kernel(const float* __restrict__ x, _Float16* __restrict__ out,
                                                                float* __restrict__ scale, float* __restrict__ norm2,
                                                                int64_t rows, int64_t d) {
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (r >= rows) return;
    const float4* src = reinterpret_cast<const float4*>(x + r * d);
    const int64_t n4 = d / 4;
    constexpr int KEEP = 8;   // rows up to 2048 floats stay in registers between the maximum and the rounding
    const bool in_regs = n4 <= 64 * KEEP;
    float4 keep[KEEP];
    float mx = 0.f;
    if (in_regs) {
#pragma unroll
        for (int u = 0; u < KEEP; ++u) {
            const int64_t c = lane + 64 * u;
            keep[u] = (c < n4) ? src[c] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int u = 0; u < KEEP; ++u) mx = row_amax4(mx, keep[u]);
    } else {
        for (int64_t c = lane; c < n4; c += 64) mx = row_amax4(mx, src[c]);
    }
    mx = wave_max(mx);
    const int e = row_scale_exponent(mx);
    const float up = ldexpf(1.f, e), down = ldexpf(1.f, -e);
    half4* dst = reinterpret_cast<half4*>(out + r * d);
    float n2 = 0.f;
    auto emit = [&](int64_t c, const float4 v) { row_pack_emit(dst, c, v, up, down, n2); };
    if (in_regs) {
#pragma unroll
        for (int u = 0; u < KEEP; ++u) {
            const int64_t c = lane + 64 * u;
            if (c < n4) emit(c, keep[u]);
        }
    } else {
        for (int64_t c = lane; c < n4; c += 64) emit(c, src[c]);
    }
    n2 = wave_sum(n2);
    if (lane == 0) {
        scale[r] = down;
        norm2[r] = n2;
    }
}

}  // namespace

int launch_pack_rows_f16(const float* x, void* out, float* scale, float* norm2, int64_t rows, int64_t d, hipStream_t st) {
    if (rows <= 0) return NW_OK;
    if ((rows + 3) / 4 > 0x7fffffffLL) return NW_ERR_INVALID_ARG;
    hipLaunchKernelGGL(nw_pack_rows_f16_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, x,
                       static_cast<_Float16*>(out), scale, norm2, rows, d);
    NW_CHECK_LAUNCH();
    return NW_OK;
}

}  // namespace nw

extern "C" int nw_pack_rows_f16(const float* x, uint16_t* out_rows, float* row_scale, float* row_norm2, int64_t rows,
                                int64_t d, void* stream) {
    if (rows < 0 || d < 0) return NW_ERR_INVALID_ARG;
    if (d % 64 != 0) return NW_ERR_UNSUPPORTED;
    if (rows == 0) return NW_OK;
    if (!x || !out_rows || !row_scale || !row_norm2) return NW_ERR_INVALID_ARG;
    if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(out_rows)) & 15) return NW_ERR_INVALID_ARG;
    return nw::launch_pack_rows_f16(x, out_rows, row_scale, row_norm2, rows, d, static_cast<hipStream_t>(stream));
}

// ------------------------------------------------------------------------------------------------------------------
// Rows of a PREPARED bank replaced in place (nw_bank_update_rows_f32): item i writes x[i] -- or, with a momentum, its blend
// with the row that was there -- to row rows[i] of the fp32 matrix and leaves every prepared form of that row as the
// kernels above (and nw_row_norm2_f32) would have made it from the new fp32 row: the same per-row functions (row_forms.h),
// the same lanes, the same order.  One wave per item, one launch, no workspace and no atomics.
// An item is skipped when its row is negative or past the bank, or when a LATER item names the same row (the wave scans
// the rest of `rows` 64 at a time): the last occurrence wins and is blended once with the old row; rows are written by one
// wave only, so there is no race.  Rows of up to 2048 floats stay in registers from the blend to the emit; longer ones are
// written to s_rows and read back by the same lane at the same index.
namespace nw {
namespace {

struct BankUpdate {
    const float* x;          // (R, dx); columns dx .. d-1 of a new row are zero
    const int64_t* rows;     // (R,)
    int64_t R, dx;
    float momentum;
    float* s_rows;           // (N, d) fp32: read (the old row of a blend) and written
    float* s_user;           // (N, dx) or null: the caller's own tensor when s_rows is the padded copy
    float* s_norm2;
    float *s_split, *s_scale;                 // both or neither
    _Float16* s_f16;                          // all three or none
    float *f16_scale, *f16_norm2;
    int64_t N, d;
    unsigned lmask;
    int vec_x;               // x may be read in 16-byte pieces (aligned, dx % 4 == 0)
};

// momentum * old + (1 - momentum) * new with the two products and the sum each rounded on their own, whatever the
// translation unit's contraction mode: what three elementwise fp32 tensor operations give
__device__ __forceinline__ float blend_rounded(float m, float om, float old, float nw_) {
#pragma clang fp contract(off)
    const float a = m * old;
    const float b = om * nw_;
    return a + b;
}

__global__ __launch_bounds__(256) void nw_bank_update_rows_kernel(const BankUpdate a) {
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (i >= a.R) return;
    const int64_t r = a.rows[i];
    if (r < 0 || r >= a.N) return;            // compared, never used as an address
    bool later = false;
    for (int64_t j = i + 1 + lane; j < a.R; j += 64) later |= a.rows[j] == r;
    if (__any(later)) return;                 // (wave-uniform: the whole wave leaves)

    const int64_t d = a.d, dx = a.dx, n4 = d / 4;
    const float* xi = a.x + i * dx;
    float* row = a.s_rows + r * d;
    const float m = a.momentum, om = 1.0f - a.momentum;
    const bool blend = m != 0.f;
    // the new row's element k / chunk c; with no momentum x's bits as they are
    auto mix = [&](float old, float nw_) { return blend_rounded(m, om, old, nw_); };
    auto elem = [&](int64_t k) -> float {
        const float v = k < dx ? xi[k] : 0.f;
        return blend ? mix(row[k], v) : v;
    };
    auto chunk = [&](int64_t c) -> float4 {
        float4 v;
        if (a.vec_x) {
            v = 4 * c < dx ? reinterpret_cast<const float4*>(xi)[c] : make_float4(0.f, 0.f, 0.f, 0.f);
        } else {
            const int64_t k = 4 * c;
            v.x = k < dx ? xi[k] : 0.f;
            v.y = k + 1 < dx ? xi[k + 1] : 0.f;
            v.z = k + 2 < dx ? xi[k + 2] : 0.f;
            v.w = k + 3 < dx ? xi[k + 3] : 0.f;
        }
        if (blend) {
            const float4 o = reinterpret_cast<const float4*>(row)[c];
            v.x = mix(o.x, v.x), v.y = mix(o.y, v.y), v.z = mix(o.z, v.z), v.w = mix(o.w, v.w);
        }
        return v;
    };
    auto store = [&](int64_t c, const float4 v) {
        reinterpret_cast<float4*>(row)[c] = v;
        if (a.s_user) {
            float* u = a.s_user + r * dx;
            const int64_t k = 4 * c;
            if (k < dx) u[k] = v.x;
            if (k + 1 < dx) u[k + 1] = v.y;
            if (k + 2 < dx) u[k + 2] = v.z;
            if (k + 3 < dx) u[k + 3] = v.w;
        }
    };
    const bool split = a.s_split != nullptr, f16 = a.s_f16 != nullptr;
    // a bank of fp16 rows keeps the PLAIN norms of its fp32 rows (nw_row_norm2_f32), which sums element k on lane k % 64:
    // gathered here from the operands, before anything of the row is written
    float plain = 0.f;
    if (!split) plain = wave_sum(row_norm2_lane(elem, d, lane));

    constexpr int KEEP = 8;
    const bool in_regs = n4 <= 64 * KEEP;
    float4 keep[KEEP];
    float mx = 0.f, n2 = 0.f;
    if (in_regs) {
#pragma unroll
        for (int u = 0; u < KEEP; ++u) {
            const int64_t c = lane + 64 * u;
            keep[u] = (c < n4) ? chunk(c) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int u = 0; u < KEEP; ++u) {
            const int64_t c = lane + 64 * u;
            if (c < n4) store(c, keep[u]);
        }
        if (split) {
#pragma unroll
            for (int u = 0; u < KEEP; ++u) row_split_accum(mx, n2, keep[u]);
        } else {
#pragma unroll
            for (int u = 0; u < KEEP; ++u) mx = row_amax4(mx, keep[u]);
        }
    } else {
        for (int64_t c = lane; c < n4; c += 64) {
            const float4 v = chunk(c);
            store(c, v);
            if (split) row_split_accum(mx, n2, v);
            else mx = row_amax4(mx, v);
        }
    }
    mx = wave_max(mx);
    const int e = row_scale_exponent(mx);
    const float up = ldexpf(1.f, e), down = ldexpf(1.f, -e);
    const float4* back = reinterpret_cast<const float4*>(row);     // (the streamed row: this lane's own stores)
    if (split) {
        n2 = wave_sum(n2);
        if (lane == 0) {
            a.s_scale[r] = down;
            a.s_norm2[r] = n2;
        }
        _Float16* dst = reinterpret_cast<_Float16*>(a.s_split + r * d);
        if (in_regs) {
#pragma unroll
            for (int u = 0; u < KEEP; ++u) {
                const int64_t c = lane + 64 * u;
                if (c < n4) row_split_emit(dst, c, keep[u], up, a.lmask);
            }
        } else {
            for (int64_t c = lane; c < n4; c += 64) row_split_emit(dst, c, back[c], up, a.lmask);
        }
    } else if (lane == 0) {
        a.s_norm2[r] = plain;
    }
    if (f16) {
        half4* dst = reinterpret_cast<half4*>(a.s_f16 + r * d);
        float hn2 = 0.f;
        if (in_regs) {
#pragma unroll
            for (int u = 0; u < KEEP; ++u) {
                const int64_t c = lane + 64 * u;
                if (c < n4) row_pack_emit(dst, c, keep[u], up, down, hn2);
            }
        } else {
            for (int64_t c = lane; c < n4; c += 64) row_pack_emit(dst, c, back[c], up, down, hn2);
        }
        hn2 = wave_sum(hn2);
        if (lane == 0) {
            a.f16_scale[r] = down;
            a.f16_norm2[r] = hn2;
        }
    }
}

}  // namespace
}  // namespace nw

extern "C" int nw_bank_update_rows_f32(const float* x, const int64_t* rows, int64_t R, int64_t dx, float momentum,
                                       float* s_rows, float* s_user, float* s_norm2, float* s_split, float* s_scale,
                                       void* s_f16, float* f16_scale, float* f16_norm2, int64_t N, int64_t d, void* stream) {
    if (R < 0 || N < 0 || d < 0) return NW_ERR_INVALID_ARG;
    if (dx < 1 || dx > d) return NW_ERR_INVALID_ARG;
    if (!(momentum >= 0.f && momentum < 1.f)) return NW_ERR_INVALID_ARG;      // (a NaN fails both)
    if (R == 0 || N == 0) return NW_OK;
    if (!x || !rows || !s_rows || !s_norm2) return NW_ERR_INVALID_ARG;
    const bool split = s_split || s_scale, f16 = s_f16 || f16_scale || f16_norm2;
    if (split && !(s_split && s_scale)) return NW_ERR_INVALID_ARG;
    if (f16 && !(s_f16 && f16_scale && f16_norm2)) return NW_ERR_INVALID_ARG;
    if ((reinterpret_cast<uintptr_t>(s_rows) | reinterpret_cast<uintptr_t>(s_split) | reinterpret_cast<uintptr_t>(s_f16)) & 15)
        return NW_ERR_INVALID_ARG;
    if (!split && !f16) return NW_ERR_UNSUPPORTED;
    if (split && d % 32 != 0) return NW_ERR_UNSUPPORTED;
    if (f16 && (d % 64 != 0 || d < 192)) return NW_ERR_UNSUPPORTED;
    if (R > 16384) return NW_ERR_UNSUPPORTED;
    const int vec_x = dx % 4 == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0;
    const nw::BankUpdate a = {x, rows, R, dx, momentum, s_rows, s_user, s_norm2, s_split, s_scale, static_cast<_Float16*>(s_f16),
                              f16_scale, f16_norm2, N, d, nw::split_lmask(), vec_x};
    hipLaunchKernelGGL(nw::nw_bank_update_rows_kernel, dim3((unsigned)((R + 3) / 4)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), a);
    NW_CHECK_LAUNCH();
    return NW_OK;
}

// ------------------------------------------------------------------------------------------------------------------
// All convolution weights of a network -> the split-row operands of conv_nhwc.hip, in ONE launch per optimizer step
// (the weights change every step; per convolution this was a permute, a flip and two split launches).
// A job reads a torch (Cout, Cin, KH, KW) contiguous weight and writes one operand:
//   mode 0  forward      rows = Cout, row co = [t][ci]               (the channels_last bytes of the weight)
//   mode 1  data grad    rows = Cin,  row ci = [T - 1 - t][co]       (flipped taps, transposed channels)
//   mode 2  few channels rows = Cout, row co = [ky][32: kx * 4 + ci] (ROWRUN4: Cin <= 4 padded to 4, a kernel row per chunk)
// jobs (device, int64 x 10 per job): src address, split offset (floats), scale offset, first row (prefix sum), rows, cols,
// Cin, Cout, T, KW | mode << 32
namespace nw {
namespace {

__global__ __launch_bounds__(256) void nw_split_conv_weights_kernel(const int64_t* __restrict__ jobs, int njobs, int64_t total_rows,
                                                                     float* __restrict__ split_base, float* __restrict__ scale_base) {
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (r >= total_rows) return;
    int lo = 0, hi = njobs - 1;                     // the job whose row range holds r
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (jobs[10 * mid + 3] <= r) lo = mid; else hi = mid - 1;
    }
    const int64_t* jb = jobs + 10 * lo;
    const float* src = reinterpret_cast<const float*>(jb[0]);
    const int row = (int)(r - jb[3]), cols = (int)jb[5], Cin = (int)jb[6], Cout = (int)jb[7], T = (int)jb[8];
    const int KW = (int)(jb[9] & 0xffffffff), mode = (int)(jb[9] >> 32);
    auto at = [&](int k) -> float {
        if (mode == 0) { const int t = k / Cin, ci = k - t * Cin; return src[((int64_t)row * Cin + ci) * T + t]; }
        if (mode == 1) { const int t = k / Cout, co = k - t * Cout; return src[((int64_t)co * Cin + row) * T + (T - 1 - t)]; }
        const int ky = k >> 5, j = k & 31, kx = j >> 2, ci = j & 3;
        return (kx < KW && ci < Cin) ? src[((int64_t)row * Cin + ci) * T + ky * KW + kx] : 0.f;
    };
    // Rows of up to 64 x 72 elements (a 3 x 3 x 512 weight's) stay in registers between the maximum and the split: the gathers of
    // the transposed (data-gradient) form are strided by Cin T floats -- every element its own cache line -- and were made twice
    // (ResNet-18: 308 -> 123 us per step).  Three register tiers, so that a short row does not walk 72 guarded slots.
    _Float16* dst = reinterpret_cast<_Float16*>(split_base + jb[1] + (int64_t)row * cols);
    auto finish = [&](float mx) {
        mx = wave_max(mx);
        int e = 0;
        if (mx > 0.f && mx < INFINITY) {
            frexpf(mx, &e);
            e = 14 - e;
            if (e > 126) e = 126;
        }
        if (lane == 0) scale_base[jb[2] + row] = ldexpf(1.f, -e);
        return ldexpf(1.f, e);
    };
    auto put = [&](int k, float x, float up) {      // element k -> half (k % 32) of the 32-k chunk k / 32; l sits 32 halves on
        const float v = x * up;
        const _Float16 h = (_Float16)v;
        dst[(k >> 5) * 64 + (k & 31)] = h;
        dst[(k >> 5) * 64 + 32 + (k & 31)] = (_Float16)(v - (float)h);
    };
    auto in_registers = [&](auto nrc) {
        constexpr int NR = decltype(nrc)::value;
        float keep[NR];
        float mx = 0.f;
#pragma unroll
        for (int j = 0; j < NR; ++j) {
            const int k = lane + 64 * j;
            keep[j] = k < cols ? at(k) : 0.f;
            mx = fmaxf(mx, fabsf(keep[j]));
        }
        const float up = finish(mx);
#pragma unroll
        for (int j = 0; j < NR; ++j) {
            const int k = lane + 64 * j;
            if (k < cols) put(k, keep[j], up);
        }
    };
    if (cols <= 64 * 8) in_registers(std::integral_constant<int, 8>{});
    else if (cols <= 64 * 24) in_registers(std::integral_constant<int, 24>{});
    else if (cols <= 64 * 72) in_registers(std::integral_constant<int, 72>{});
    else {
        float mx = 0.f;
        for (int k = lane; k < cols; k += 64) mx = fmaxf(mx, fabsf(at(k)));
        const float up = finish(mx);
        for (int k = lane; k < cols; k += 64) put(k, at(k), up);
    }
}

}  // namespace
}  // namespace nw

extern "C" int nw_split_conv_weights_f16x2(const int64_t* jobs, int64_t njobs, int64_t total_rows, float* split_base,
                                           float* scale_base, void* stream) {
    if (njobs < 0 || total_rows < 0) return NW_ERR_INVALID_ARG;
    if (njobs == 0 || total_rows == 0) return NW_OK;
    if (!jobs || !split_base || !scale_base || njobs > 0x7fffffffLL) return NW_ERR_INVALID_ARG;
    hipLaunchKernelGGL(nw::nw_split_conv_weights_kernel, dim3((unsigned)((total_rows + 3) / 4)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), jobs, (int)njobs, total_rows, split_base, scale_base);
    NW_CHECK_LAUNCH();
    return NW_OK;
}
