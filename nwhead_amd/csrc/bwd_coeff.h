// bwd_coeff.h -- the per-pair coefficients of the head's backward, shared by the coefficient kernel of the score-matrix
// route (backward.hip, nw_bwd_coeff_kernel) and the fused query gradient over a resident bank (bwd_query.hip).
//
// For a score s = f(dot, |q|^2, |s|^2) and dS = W (dW - t) (backward.hip's closed form):
//     a = dS df/ddot        rq += dS df/d|q|^2        r = dS df/d|s|^2        gls += dS df/dlogit_scale  (clip)
// Euclidean: df/ddot = 1/D, df/d|q|^2 = df/d|s|^2 = -1/(2D), all 0 where D == 0 (torch's cdist backward masks the zero
// distance the same way).  The cosine-type kinds go through F.normalize, whose clamp at NW_NORM_EPS passes no gradient
// through the norm of a row below it.
#pragma once
#include "nw_internal.h"

namespace nw {

// What depends on the query alone: the clip scale, max(|q|, eps) and 1 / max(|q|, eps)^2 (0 below the clamp).
template <int KIND>
__device__ __forceinline__ void bwd_query_factors(float qn2, const float* __restrict__ logit_scale, float& scale, float& nq,
                                                  float& inq2) {
    scale = 1.f, nq = 1.f, inq2 = 0.f;
    if (KIND == NW_SCORE_CLIP) scale = expf(*logit_scale);
    if (KIND == NW_SCORE_HYPERSPHERE || KIND == NW_SCORE_COSINE || KIND == NW_SCORE_CLIP) {
        const float n = sqrtf(qn2);
        nq = fmaxf(n, NW_NORM_EPS);
        inq2 = (n > NW_NORM_EPS) ? 1.f / (nq * nq) : 0.f;  // F.normalize clamps: no grad via |q|
    }
}

// One (query, support) pair: `sc` its score in natural units, `sn2v` the support's squared norm (read by the cosine-type
// kinds only).  a and r are returned, the query's sums rq_acc / gls_acc are added to.
template <int KIND>
__device__ __forceinline__ void bwd_pair_coeff(float sc, float dS, float sn2v, float scale, float nq, float inq2, float& a,
                                               float& r, float& rq_acc, float& gls_acc) {
    if (KIND == NW_SCORE_DOT) {
        a = dS;
        r = 0.f;
    } else if (KIND == NW_SCORE_EUCLIDEAN) {
        const float D = -sc;
        a = (D == 0.f) ? 0.f : dS / D;
        r = -0.5f * a;
        rq_acc += r;
    } else {
        const float sn = sqrtf(sn2v);
        const float ns = fmaxf(sn, NW_NORM_EPS);
        const float ins2 = (sn > NW_NORM_EPS) ? 1.f / (ns * ns) : 0.f;
        float fc, c;  // df/dcos and cos
        if (KIND == NW_SCORE_HYPERSPHERE) {
            const float D = -sc;
            fc = (D == 0.f) ? 0.f : 1.f / D;
            c = 1.f - 0.5f * D * D;
        } else {
            fc = scale;
            c = sc / scale;
            gls_acc += dS * sc;  // d(e^ls cos)/d ls = score
        }
        const float gc = dS * fc;
        a = gc / (nq * ns);
        rq_acc += gc * (-0.5f * c * inq2);
        r = gc * (-0.5f * c * ins2);
    }
}

}  // namespace nw
