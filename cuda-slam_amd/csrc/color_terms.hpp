// K48 / K49 building blocks: the colour gradient of a point from its neighbourhood's sums and the terms of one colored-ICP pair, usable
// from one GPU lane and from host code (color_kernels.hip; tests/color_terms_selftest.cpp compiles this header alone with a host compiler).
// The rules are those of include/mi_slam.h (mi_estimate_color_gradients, mi_icp_color_register), operation for operation: every operand
// is a double, every operation is rounded (the build has -ffp-contract=off; a host build needs the same), sums of three are formed left to
// right, a cofactor and a cross-product component are two products and one subtraction.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MISLAM_COLOR_HD __host__ __device__
#else
#define MISLAM_COLOR_HD
#endif

#include <cfloat>

namespace mislam {

// One neighbour of the gradient's least squares: e = p_j - p_i, delta = I_j - I_i, n the point's normal.  u = e - (n . e) n is the
// neighbour in the tangent plane; M += u u^T on the six upper entries (xx, xy, xz, yy, yz, zz), b += u delta.
MISLAM_COLOR_HD inline void color_gradient_add(const double (&n)[3], double ex, double ey, double ez, double delta, double (&M)[6], double (&b)[3])
{
    const double s = (n[0] * ex + n[1] * ey) + n[2] * ez;
    const double ux = ex - s * n[0], uy = ey - s * n[1], uz = ez - s * n[2];
    M[0] += ux * ux; M[1] += ux * uy; M[2] += ux * uz;
    M[3] += uy * uy; M[4] += uy * uz; M[5] += uz * uz;
    b[0] += ux * delta; b[1] += uy * delta; b[2] += uz * delta;
}

// The constraint d . n = 0 as one more row of the least squares, weighted by the neighbour count: M_ab += ((w w) n_a) n_b, w = (double)count.
MISLAM_COLOR_HD inline void color_gradient_constrain(const double (&n)[3], int count, double (&M)[6])
{
    const double w = (double)count;
    const double ww = w * w;
    const double a0 = ww * n[0], a1 = ww * n[1], a2 = ww * n[2];
    M[0] += a0 * n[0]; M[1] += a0 * n[1]; M[2] += a0 * n[2];
    M[3] += a1 * n[1]; M[4] += a1 * n[2]; M[5] += a2 * n[2];
}

// d = M^-1 b by the adjugate and the determinant.  false, and d = (0, 0, 0): a det that is <= 0 or not finite.
MISLAM_COLOR_HD inline bool color_gradient_solve(const double (&M)[6], const double (&b)[3], double (&d)[3])
{
    const double c00 = M[3] * M[5] - M[4] * M[4], c01 = M[2] * M[4] - M[1] * M[5], c02 = M[1] * M[4] - M[2] * M[3];
    const double c11 = M[0] * M[5] - M[2] * M[2], c12 = M[1] * M[2] - M[0] * M[4], c22 = M[0] * M[3] - M[1] * M[1];
    const double det = (M[0] * c00 + M[1] * c01) + M[2] * c02;
    if (!(det > 0.0 && det <= DBL_MAX)) { d[0] = 0.0; d[1] = 0.0; d[2] = 0.0; return false; }
    d[0] = ((c00 * b[0] + c01 * b[1]) + c02 * b[2]) / det;
    d[1] = ((c01 * b[0] + c11 * b[1]) + c12 * b[2]) / det;
    d[2] = ((c02 * b[0] + c12 * b[1]) + c22 * b[2]) / det;
    return true;
}

// What a lane keeps of its pair: the two Jacobian rows and residuals.  All zeros: no pair, every entry below is +0.
struct ColorPair {
    double JG[6], JC[6], rG, rC;
};

MISLAM_COLOR_HD inline void color_pair_none(ColorPair& p)
{
    for (int i = 0; i < 6; i++) { p.JG[i] = 0.0; p.JC[i] = 0.0; }
    p.rG = 0.0; p.rC = 0.0;
}

// q: the moved point; a, n, g, Ia: the matched fixed point, its normal, colour gradient and intensity; Ib: the moving point's intensity;
// c0: the centre.  dv = q - a, P = q - c0, rG = n . dv, JG = [P x n, n]; qp = dv - rG n, rC = ((g . qp) + Ia) - Ib, mvec = g - (g . n) n,
// JC = [P x mvec, mvec].
MISLAM_COLOR_HD inline void color_pair_terms(const double (&q)[3], const double (&a)[3], const double (&c0)[3], const double (&n)[3], const double (&g)[3],
                                             double Ia, double Ib, ColorPair& p)
{
    const double dx = q[0] - a[0], dy = q[1] - a[1], dz = q[2] - a[2];
    const double px = q[0] - c0[0], py = q[1] - c0[1], pz = q[2] - c0[2];
    const double rG = (n[0] * dx + n[1] * dy) + n[2] * dz;
    p.rG = rG;
    p.JG[0] = py * n[2] - pz * n[1]; p.JG[1] = pz * n[0] - px * n[2]; p.JG[2] = px * n[1] - py * n[0];
    p.JG[3] = n[0]; p.JG[4] = n[1]; p.JG[5] = n[2];
    const double qx = dx - rG * n[0], qy = dy - rG * n[1], qz = dz - rG * n[2];
    p.rC = (((g[0] * qx + g[1] * qy) + g[2] * qz) + Ia) - Ib;
    const double gn = (g[0] * n[0] + g[1] * n[1]) + g[2] * n[2];
    const double mx = g[0] - gn * n[0], my = g[1] - gn * n[1], mz = g[2] - gn * n[2];
    p.JC[0] = py * mz - pz * my; p.JC[1] = pz * mx - px * mz; p.JC[2] = px * my - py * mx;
    p.JC[3] = mx; p.JC[4] = my; p.JC[5] = mz;
}

// The row's entries of the pair under the weights lg = (double)lambda_geometric and lc = 1.0 - lg
MISLAM_COLOR_HD inline double color_pair_h(const ColorPair& p, double lg, double lc, int i, int j) { return lg * (p.JG[i] * p.JG[j]) + lc * (p.JC[i] * p.JC[j]); }
MISLAM_COLOR_HD inline double color_pair_g(const ColorPair& p, double lg, double lc, int i) { return lg * (p.JG[i] * p.rG) + lc * (p.JC[i] * p.rC); }
MISLAM_COLOR_HD inline double color_pair_e(const ColorPair& p, double lg, double lc) { return lg * (p.rG * p.rG) + lc * (p.rC * p.rC); }

}  // namespace mislam
