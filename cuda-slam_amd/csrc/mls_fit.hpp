// K50 building block: what mi_mls_smooth does with the sums of its two walks, usable from one GPU lane and from host code (the lane of
// mls_kernels.hip; tests/mls_fit_selftest.cpp compiles this header alone with a host compiler).  The single statement of the rules mi_slam.h
// gives under "Plane", "Frame", "Quadratic" and "Outputs"; everything is fp64.
//
//   mls_plane     S = sum d, Q = sum d d^T over the c points of the ball -> the covariance (m = S / c, C = Q / c - m m^T), its eigenvalues and the
//                 unit eigenvector n of the smallest (eig3.hpp, normalised as mi_estimate_normals does), the curvature, the query's foot on
//                 the plane o = ((n . m)) n, and the frame.
//   mls_frame     k = the axis with the smallest |n_k|, the lowest on ties; u = (e_k x n) / |e_k x n|, v = n x u.  |e_k x n|^2 = 1 - n_k^2 >= 2 / 3.
//   mls_basis     one point of the ball into the 21 + 6 sums: e = d - o, a = u . e, b = v . e, f = n . e, w = exp(-(d . d) / s2),
//                 phi = (1, a, b, a a, a b, b b), A_ij += (w phi_i) phi_j (i <= j, row by row), g_i += (w phi_i) f.
//   mls_project   the fall-back decision and the projection: the quadratic where order == 2, c >= MLS_QUADRATIC_MIN and plane_solve6
//                 (plane_solve.hpp: the same scaling, the same pivot floor, the same verdict) accepts the system; the plane otherwise.
// Every loop has constant bounds and is unrolled on the device, so every index is static there.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MISLAM_MLS_HD __host__ __device__
#define MISLAM_MLS_UNROLL _Pragma("unroll")
#else
#define MISLAM_MLS_HD
#define MISLAM_MLS_UNROLL
#endif

#include <cmath>

#include "eig3.hpp"
#include "plane_solve.hpp"

namespace mislam {

constexpr int MLS_QUADRATIC_MIN = 6;          // fewer points than coefficients: the plane
constexpr int MLS_QUADRATIC = 0, MLS_PLANE = 1, MLS_UNTOUCHED = 2;       // MI_MLS_* (mi_slam.h)

struct MlsPlane {
    double n[3], o[3], u[3], v[3];             // the unit normal, the query's foot relative to the query, the frame
    double lambda[3];                          // ascending
    double curvature;
};

MISLAM_MLS_HD inline void mls_frame(const double (&n)[3], double (&u)[3], double (&v)[3])
{
    using std::fabs;
    using std::sqrt;
    const double ax = fabs(n[0]), ay = fabs(n[1]), az = fabs(n[2]);
    const bool k0 = ax <= ay && ax <= az, k1 = !k0 && ay <= az;                 // (the lowest axis of a tie)
    // e_x x n = (0, -n_z, n_y); e_y x n = (n_z, 0, -n_x); e_z x n = (-n_y, n_x, 0)
    const double x = k0 ? 0.0 : (k1 ? n[2] : -n[1]);
    const double y = k0 ? -n[2] : (k1 ? 0.0 : n[0]);
    const double z = k0 ? n[1] : (k1 ? -n[0] : 0.0);
    const double len = sqrt((x * x + y * y) + z * z);
    u[0] = x / len; u[1] = y / len; u[2] = z / len;
    v[0] = n[1] * u[2] - n[2] * u[1];
    v[1] = n[2] * u[0] - n[0] * u[2];
    v[2] = n[0] * u[1] - n[1] * u[0];
}

// S: sum d; Q: sum d d^T (xx, xy, xz, yy, yz, zz); c >= 1 points
MISLAM_MLS_HD inline void mls_plane(const double (&S)[3], const double (&Q)[6], int c, MlsPlane& p)
{
    using std::sqrt;
    const double cd = (double)c;
    const double mx = S[0] / cd, my = S[1] / cd, mz = S[2] / cd;
    const double cov[6] = {Q[0] / cd - mx * mx, Q[1] / cd - mx * my, Q[2] / cd - mx * mz, Q[3] / cd - my * my, Q[4] / cd - my * mz, Q[5] / cd - mz * mz};
    double v[9];
    eig3_symmetric<double>(cov, p.lambda, v);
    double nx = v[0], ny = v[3], nz = v[6];
    const double len = sqrt((nx * nx + ny * ny) + nz * nz);                       // (1 to rounding: V is a product of rotations)
    nx /= len; ny /= len; nz /= len;
    p.n[0] = nx; p.n[1] = ny; p.n[2] = nz;
    const double sum = (p.lambda[0] + p.lambda[1]) + p.lambda[2];
    p.curvature = sum > 0.0 ? (p.lambda[0] > 0.0 ? p.lambda[0] : 0.0) / sum : 0.0;
    const double t = (nx * mx + ny * my) + nz * mz;
    p.o[0] = t * nx; p.o[1] = t * ny; p.o[2] = t * nz;
    mls_frame(p.n, p.u, p.v);
}

// d = p_j - q; s2: the square of the Gaussian's scale
MISLAM_MLS_HD inline void mls_basis(const MlsPlane& p, double dx, double dy, double dz, double s2, double (&A)[21], double (&g)[6])
{
    using std::exp;
    const double ex = dx - p.o[0], ey = dy - p.o[1], ez = dz - p.o[2];
    const double a = (p.u[0] * ex + p.u[1] * ey) + p.u[2] * ez;
    const double b = (p.v[0] * ex + p.v[1] * ey) + p.v[2] * ez;
    const double f = (p.n[0] * ex + p.n[1] * ey) + p.n[2] * ez;
    const double w = exp(-(((dx * dx + dy * dy) + dz * dz) / s2));
    const double phi[6] = {1.0, a, b, a * a, a * b, b * b};
    int k = 0;
    MISLAM_MLS_UNROLL
    for (int i = 0; i < 6; i++) {
        const double wp = w * phi[i];
        MISLAM_MLS_UNROLL
        for (int j = i; j < 6; j++) { A[k] += wp * phi[j]; k++; }
        g[i] += wp * f;
    }
}

// q: the query; c: the points of its ball (>= 1); A, g: read where order == 2 and c >= MLS_QUADRATIC_MIN only.  Returns MLS_QUADRATIC or
// MLS_PLANE; xyz and normal unrounded.  min_pivot (may be null): plane_solve6's, 0 where it did not run.
MISLAM_MLS_HD inline int mls_project(const MlsPlane& p, const double (&q)[3], int order, int c, const double (&A)[21], const double (&g)[6],
                                     double (&xyz)[3], double (&normal)[3], double* min_pivot)
{
    using std::sqrt;
    if (min_pivot) *min_pivot = 0.0;
    if (order == 2 && c >= MLS_QUADRATIC_MIN) {
        double x[6];
        if (plane_solve6(A, g, x, min_pivot)) {                                      // A x = -g: the coefficients are -x
            const double c0 = -x[0], c1 = -x[1], c2 = -x[2];
            double m[3];
            MISLAM_MLS_UNROLL
            for (int k = 0; k < 3; k++) {
                xyz[k] = (q[k] + p.o[k]) + c0 * p.n[k];
                m[k] = (p.n[k] - c1 * p.u[k]) - c2 * p.v[k];
            }
            const double len = sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]);      // (>= 1: n is a unit vector orthogonal to u and v)
            MISLAM_MLS_UNROLL
            for (int k = 0; k < 3; k++) normal[k] = m[k] / len;
            return MLS_QUADRATIC;
        }
    }
    MISLAM_MLS_UNROLL
    for (int k = 0; k < 3; k++) { xyz[k] = q[k] + p.o[k]; normal[k] = p.n[k]; }
    return MLS_PLANE;
}

}  // namespace mislam
