// The arithmetic of an exact-P EM iteration that more than one translation unit evaluates: the Gaussian affinity, the state at sigma^2_0,
// the M-step's one-lane solve with the EM stop rule, the transform.  Included by cpd_kernels.hip (one registration over the whole device)
// and cpd_batch.hip (one workgroup per registration), so that both run the same operations in the same order: with -ffp-contract=off every
// rounding below is written out, and what is written once cannot drift apart.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "cpd_kernels.h"
#include "svd3.hpp"

namespace mislam {

__device__ __forceinline__ float sq_dist(float ax, float ay, float az, float bx, float by, float bz)
{
    const float dx = ax - bx, dy = ay - by, dz = az - bz;   // cloudAfter[x] - cloudTransformed[k], coherentpointdrift.cpp:190
    return (dx * dx + dy * dy) + dz * dz;
}

// exp(x) for the Gaussian affinities (x <= 0).  The libm-grade expf the compiler inlines costs ~17 VALU issue slots per call
// (range reduction, ldexp, overflow/underflow selects) and is >60 % of a pair; this one is 9: the exponent x*log2(e) is formed
// as a rounded product h plus its exact residual (fma) plus the low part of log2(e), 2^h comes from v_exp_f32 (1 ulp) and the
// residual is applied to first order, 2^(h+r) = 2^h (1 + r ln 2) with |r| < 2^-23 |h|.  Max relative error ~2 ulp against
// glibc's expf over [-104, 0]; results below FLT_MIN flush to zero (they add to a denominator >= c, c ~ 1e1..1e2).
#ifndef MISLAM_CPD_EXP_FORM
#define MISLAM_CPD_EXP_FORM 2              // 2: compensated (the text above); 0: v_exp_f32(x * log2 e) alone -- measurement only
#endif
__device__ __forceinline__ float exp_neg(float x)
{
    const float L_hi = 1.44269502162933349609375f;     // float(log2 e)
    const float h = x * L_hi;
#if MISLAM_CPD_EXP_FORM == 0
    return __builtin_amdgcn_exp2f(h);
#else
    const float L_lo = 1.925963033500011e-08f;         // log2 e - L_hi
    float r = __builtin_fmaf(x, L_hi, -h);
    r = __builtin_fmaf(x, L_lo, r);
    const float e = __builtin_amdgcn_exp2f(h);
    return __builtin_fmaf(e * r, 0.693147182464599609375f, e);
#endif
}

// One Gaussian affinity from its exponent.  TRUNC: the hybrid mode's truncated kernel (coherentpointdrift.cpp:193-196) --
// an exponent below log(truncate) contributes exactly 0 to the denominator and to P1/PX.
template <bool TRUNC>
__device__ __forceinline__ float affinity(float index, float trunc_log)
{
    if (TRUNC) return index < trunc_log ? 0.f : exp_neg(index);
    return exp_neg(index);
}

// The same affinity for TWO fixed points at once, as packed fp32 operations (v_pk_add_f32 / v_pk_mul_f32 / v_pk_fma_f32: the same IEEE
// operations, two results per issue slot -- bit for bit what two calls of affinity() return).  The two points' coordinates are register
// PAIRS straight out of the batched scalar loads; only the two v_exp_f32 stay single.
typedef float cpd_f32x2 __attribute__((ext_vector_type(2)));
template <bool TRUNC>
__device__ __forceinline__ cpd_f32x2 affinity2(float mult, cpd_f32x2 ax, cpd_f32x2 ay, cpd_f32x2 az, float bx, float by, float bz, float trunc_log)
{
    const cpd_f32x2 dx = ax - (cpd_f32x2){bx, bx}, dy = ay - (cpd_f32x2){by, by}, dz = az - (cpd_f32x2){bz, bz};
    const cpd_f32x2 d = (dx * dx + dy * dy) + dz * dz;
    const cpd_f32x2 x = (cpd_f32x2){mult, mult} * d;
    const cpd_f32x2 L_hi = {1.44269502162933349609375f, 1.44269502162933349609375f}, L_lo = {1.925963033500011e-08f, 1.925963033500011e-08f};
    const cpd_f32x2 ln2 = {0.693147182464599609375f, 0.693147182464599609375f};
    const cpd_f32x2 h = x * L_hi;
    const cpd_f32x2 e = {__builtin_amdgcn_exp2f(h.x), __builtin_amdgcn_exp2f(h.y)};
#if MISLAM_CPD_EXP_FORM == 0
    cpd_f32x2 p = e;
    (void)L_lo; (void)ln2;
#else
    cpd_f32x2 r = __builtin_elementwise_fma(x, L_hi, -h);
    r = __builtin_elementwise_fma(x, L_lo, r);
    cpd_f32x2 p = __builtin_elementwise_fma(e * r, ln2, e);
#endif
    if (TRUNC) { p.x = x.x < trunc_log ? 0.f : p.x; p.y = x.y < trunc_log ? 0.f : p.y; }
    return p;
}

typedef float f32x4 __attribute__((ext_vector_type(4)));

// The state before the first iteration, from the eight sums of the two clouds (one lane; s = { sum a (3), sum |a|^2, sum b (3), sum |b|^2 }).
__device__ __forceinline__ void cpd_init_state_body(CpdState* __restrict__ st, const double (&s)[CPD_INIT_SUMS], const CpdRules& rules,
                                                    float sigma2_override, int sigma2_from_state)
{
    for (int i = 0; i < CPD_INIT_SUMS; i++) st->init[i] = s[i];
    const double M = rules.m, N = rules.n;
    const double total = N * s[7] + M * s[3] - 2.0 * (s[0] * s[4] + s[1] * s[5] + s[2] * s[6]);
    float sigma2 = (float)(total / (3.0 * M * N));
    if (sigma2_override > 0.f) sigma2 = sigma2_override;
    else if (sigma2_from_state) sigma2 = st->sigma2_init;
    for (int i = 0; i < 9; i++) st->R[i] = (i % 4 == 0) ? 1.f : 0.f;
    st->t[0] = st->t[1] = st->t[2] = 0.f;
    st->scale = 1.f;
    st->sigma2 = sigma2;
    st->sigma2_init = sigma2;
    // constant = (pow(2*M_PI*sigma2, 1.5) * weight * |before|) / ((1 - weight) * |after|)   coherentpointdrift.cpp:98:
    // the pow and the numerator are double, the denominator a float product, the quotient narrowed to float
    const double num = pow(2.0 * 3.14159265358979323846 * (double)sigma2, 1.5) * (double)rules.weight * M;
    const float den = (1.f - rules.weight) * (float)rules.n;
    st->constant = (float)(num / (double)den);
    st->L = 0.f;
    st->l_prev = 0.f;
    st->ntol = rules.tolerance + 10.0f;      // :99
    st->error = 1e5f;                        // :86
    st->Np = 0.f;
    st->iterations = 0;
    st->stop_reason = MI_STOP_RUNNING_;
    // loop condition, evaluated before the first iteration (:106)
    st->done = 0;
    if (!(0 < rules.max_iterations)) { st->done = 1; st->stop_reason = MI_STOP_MAX_ITERATIONS_; }
    else if (!(sigma2 > rules.eps)) { st->done = 1; st->stop_reason = MI_STOP_SIGMA_; }
}

// The M-step from its reduced moments, on one lane (xs, ks: cpd_kernels.hip K8), and -- with update_loop_state -- the EM bookkeeping.
__device__ __forceinline__ void cpd_solve_body(CpdState* __restrict__ st, const double (&xs)[CPD_XSUMS], const double (&ks)[CPD_KSUMS],
                                               const CpdRules& rules, int update_loop_state)
{
    for (int i = 0; i < CPD_XSUMS; i++) st->xs[i] = xs[i];
    for (int i = 0; i < CPD_KSUMS; i++) st->ks[i] = ks[i];

    float sigma2 = st->sigma2;
    if (update_loop_state) {
        // error = -sum log den + DIMENSION*N*log(sigma2)/2   coherentpointdrift.cpp:215-217
        const float L = (float)(-xs[0]) + (float)(3 * rules.n) * logf(sigma2) / 2.0f;
        st->ntol = fabsf((L - st->l_prev) / L);        // :114
        st->l_prev = L;
        st->L = L;
    }
    // ---- MStep, coherentpointdrift.cpp:223-277
    const float Np = (float)ks[0];
    const float InvertedNp = 1.0f / Np;
    float cb[3], ca[3];
    for (int d = 0; d < 3; d++) {
        cb[d] = (float)((double)InvertedNp * ks[1 + d]);      // InvertedNp * EigenBefore * p1
        ca[d] = (float)((double)InvertedNp * xs[1 + d]);      // InvertedNp * EigenAfter * pt1
    }
    Mat3 A;   // (EigenBefore * px)^T - Np * centerAfter * centerBefore^T
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) A.a[r][c] = (float)ks[4 + 3 * c + r] - Np * (ca[r] * cb[c]);
    const Kabsch3 kb = kabsch_rotation<true>(A, rules.svd_ieee != 0);     // (svd3.hpp SvdMath: the one-lane chain, as in the ICP solve)
    const float scaleNumerator = (kb.S[0] + kb.S[1]) + kb.S[2] * kb.det;
    const float sigmaSubtrahend = (float)xs[4] - Np * ((ca[0] * ca[0] + ca[1] * ca[1]) + ca[2] * ca[2]);
    const float scaleDenominator = (float)ks[13] - Np * ((cb[0] * cb[0] + cb[1] * cb[1]) + cb[2] * cb[2]);
    float scale = st->scale;
    if (!rules.const_scale) {
        scale = scaleNumerator / scaleDenominator;
        sigma2 = (InvertedNp * fabsf(sigmaSubtrahend - scale * scaleNumerator)) / 3.f;
    } else {
        sigma2 = (InvertedNp * fabsf(sigmaSubtrahend + scaleDenominator - 2 * scaleNumerator)) / 3.f;
    }
    for (int i = 0; i < 3; i++) {
        const float rc = ((kb.R.a[i][0] * scale) * cb[0] + (kb.R.a[i][1] * scale) * cb[1]) + (kb.R.a[i][2] * scale) * cb[2];
        st->t[i] = ca[i] - rc;
    }
    for (int c = 0; c < 3; c++)
        for (int r = 0; r < 3; r++) st->R[3 * c + r] = kb.R.a[r][c];
    st->scale = scale;
    st->sigma2 = sigma2;
    st->Np = Np;
    if (update_loop_state) {
        st->error = sigma2;                            // :121
        st->iterations += 1;
        // while (iterations < maxIterations && ntol > tolerance && sigmaSquared > eps)   :106
        if (!(st->iterations < rules.max_iterations)) { st->done = 1; st->stop_reason = MI_STOP_MAX_ITERATIONS_; }
        else if (!(st->ntol > rules.tolerance)) { st->done = 1; st->stop_reason = MI_STOP_TOLERANCE_; }
        else if (!(sigma2 > rules.eps)) { st->done = 1; st->stop_reason = MI_STOP_SIGMA_; }
    }
}

// y = scale * (R * b) + t   (TransformPoint with scale, common.cpp:51-55; glm operation order)
__device__ __forceinline__ void cpd_transform_point(const CpdState* st, float x, float y, float z, float* ox, float* oy, float* oz)
{
    const float s = st->scale;
    *ox = s * ((st->R[0] * x + st->R[3] * y) + st->R[6] * z) + st->t[0];
    *oy = s * ((st->R[1] * x + st->R[4] * y) + st->R[7] * z) + st->t[1];
    *oz = s * ((st->R[2] * x + st->R[5] * y) + st->R[8] * z) + st->t[2];
}

}  // namespace mislam
