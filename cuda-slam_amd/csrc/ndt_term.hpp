// K27 building block: the term of one (moved point, voxel) pair of the NDT registration (mi_ndt_register; mi_slam.h states the rule),
// usable from one GPU lane and from host code (tests/ndt_term_selftest.cpp compiles this header alone with a host compiler).
//
// Every operand is fp64 (the caller promotes the fp32 point, mean and information matrix), every operation is rounded on its own
// (-ffp-contract=off) and sums of three are formed left to right:
//   d = q - mu;  Md_r = (M_r0 d_x + M_r1 d_y) + M_r2 d_z;  m = (d_x Md_0 + d_y Md_1) + d_z Md_2;  e = exp(h m);  w = k e
// with h = -d2 / 2 and k = -(d1 d2) of mi_ndt_constants.  No term: all six entries of M are zero (a voxel without a distribution), or
// m is negative or not finite (an indefinite matrix handed in by the caller).
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MISLAM_NDT_HD __host__ __device__
#else
#define MISLAM_NDT_HD
#endif

#include <cfloat>
#include <cmath>

namespace mislam {

struct NdtTerm {
    double d[3];             // q - mu
    double Md[3];            // M d
    double m;                // d^T M d
    double e, w;             // exp(h m), k e
};

// M = {xx, xy, xz, yy, yz, zz}.  false: the pair has no term (out is then unspecified).
MISLAM_NDT_HD inline bool ndt_term(const double q[3], const double mu[3], const double M[6], double h, double k, NdtTerm* out)
{
    using std::exp;
    if (M[0] == 0.0 && M[1] == 0.0 && M[2] == 0.0 && M[3] == 0.0 && M[4] == 0.0 && M[5] == 0.0) return false;
    const double dx = q[0] - mu[0], dy = q[1] - mu[1], dz = q[2] - mu[2];
    const double Md0 = (M[0] * dx + M[1] * dy) + M[2] * dz;
    const double Md1 = (M[1] * dx + M[3] * dy) + M[4] * dz;
    const double Md2 = (M[2] * dx + M[4] * dy) + M[5] * dz;
    const double m = (dx * Md0 + dy * Md1) + dz * Md2;
    if (!(m >= 0.0 && m <= DBL_MAX)) return false;                              // (false for NaN)
    const double e = exp(h * m);
    out->d[0] = dx; out->d[1] = dy; out->d[2] = dz;
    out->Md[0] = Md0; out->Md[1] = Md1; out->Md[2] = Md2;
    out->m = m; out->e = e; out->w = k * e;
    return true;
}

// What a point keeps of its voxels' terms: A = sum w M, b = sum w Md, E = sum e, in the order the terms come (one product and one
// addition per entry and term).  From A and b the 27 entries of the point's H and g are formed once, as K17 forms them from M and Md.
struct NdtPointSums {
    double A[6], b[3], E;
    int terms;
};

MISLAM_NDT_HD inline void ndt_point_clear(NdtPointSums* s)
{
    for (int i = 0; i < 6; i++) s->A[i] = 0.0;
    for (int i = 0; i < 3; i++) s->b[i] = 0.0;
    s->E = 0.0;
    s->terms = 0;
}

MISLAM_NDT_HD inline void ndt_point_add(NdtPointSums* s, const double M[6], const NdtTerm& t)
{
    for (int i = 0; i < 6; i++) s->A[i] += t.w * M[i];
    for (int i = 0; i < 3; i++) s->b[i] += t.w * t.Md[i];
    s->E += t.e;
    s->terms++;
}

// The constants of the score (Magnusson 2009, eq. 6.8; PCL's gauss_d1 and gauss_d2), fp64, r the voxel size and o the outlier ratio:
// out = d1, d2, h = -0.5 d2, k = -(d1 d2).
inline void ndt_constants(double r, double o, double out[4])
{
    const double c1 = 10.0 * (1.0 - o);
    const double c2 = o / ((r * r) * r);
    const double d3 = -std::log(c2);
    const double d1 = -std::log(c1 + c2) - d3;
    const double d2 = -2.0 * std::log((-std::log(c1 * std::exp(-0.5) + c2) - d3) / d1);
    out[0] = d1; out[1] = d2; out[2] = -0.5 * d2; out[3] = -(d1 * d2);
}

}  // namespace mislam
