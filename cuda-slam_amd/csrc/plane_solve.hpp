// K16 building block: the 6 x 6 solve and the pose update of a point-to-plane ICP iteration (mi_icp_plane_register), usable from one GPU
// lane and from host code (the solve lane of plane_kernels.hip; tests/plane_solve_selftest.cpp compiles this header alone with a host
// compiler).  The single statement of the rules mi_slam.h gives under "Solve" and "Update"; everything is fp64.
//
//   plane_solve6     A = sum J J^T (upper triangle, row-major, 21 numbers) and g = sum J r (6 numbers) -> x = (omega, v) with A x = -g.
//                    Any diagonal entry <= 0 or not finite: degenerate (an exact plane has diagonal entries that are exactly 0).  Otherwise
//                    S = D^-1/2 A D^-1/2 has a unit diagonal, and LDL^T without pivoting runs on S: every pivot is then a number between 0 and
//                    1 that says how much of that motion the motions before it leave undetermined, whatever the clouds' units.  A pivot below
//                    PLANE_PIVOT_MIN (or NaN): degenerate.  Forward substitution, the diagonal, back substitution, and the scaling undone.
//   plane_rodrigues  dR = exp([omega]x) = I + a K + b K^2, a = sin(th) / th, b = (1 - cos(th)) / th^2 = 2 sin^2(th / 2) / th^2, th = |omega|; below th = 1e-8 the
//                    series a = 1 - th^2 / 6, b = 1 / 2 - th^2 / 24 (their next terms are below 2^-53 there).
//   plane_compose    R <- dR R, t <- dR (t - c0) + c0 + v: the increment turns about the centre c0 the moments were taken about.
// Matrices are row-major.  Every loop has constant bounds and is unrolled on the device, so every index is static there.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MISLAM_PLANE_HD __host__ __device__
#define MISLAM_PLANE_UNROLL _Pragma("unroll")
#else
#define MISLAM_PLANE_HD
#define MISLAM_PLANE_UNROLL
#endif

#include <cmath>

namespace mislam {

constexpr double PLANE_PIVOT_MIN = 1e-10;     // of the scaled system's LDL^T; a well-constrained scene has a smallest pivot of about 0.6
constexpr double PLANE_SERIES_BELOW = 1e-8;   // |omega| under which Rodrigues' coefficients come from their series
constexpr int PLANE_MIN_PAIRS = 6;            // fewer pairs than unknowns: MI_STOP_NO_PAIRS

// false: degenerate, x is not written.  min_pivot (may be null): the smallest pivot met, the failing one included; 0 for a bad diagonal.
MISLAM_PLANE_HD inline bool plane_solve6(const double (&A21)[21], const double (&g)[6], double (&x)[6], double* min_pivot)
{
    using std::sqrt;
    double S[6][6], inv_root[6];
    if (min_pivot) *min_pivot = 0.0;
    {
        int k = 0;
        MISLAM_PLANE_UNROLL
        for (int i = 0; i < 6; i++) {
            MISLAM_PLANE_UNROLL
            for (int j = i; j < 6; j++) { S[i][j] = A21[k]; S[j][i] = A21[k]; k++; }
        }
    }
    bool usable = true;
    MISLAM_PLANE_UNROLL
    for (int i = 0; i < 6; i++) {
        const double d = S[i][i];
        if (!(d > 0.0) || !(d <= 1.7976931348623157e308)) usable = false;
        inv_root[i] = 1.0 / sqrt(d);
    }
    if (!usable) return false;
    MISLAM_PLANE_UNROLL
    for (int i = 0; i < 6; i++) {
        MISLAM_PLANE_UNROLL
        for (int j = 0; j < 6; j++) S[i][j] = i == j ? 1.0 : (S[i][j] * inv_root[i]) * inv_root[j];
    }
    // S = L D L^T, L unit lower triangular (kept below S's diagonal), D in piv
    double piv[6], smallest = 1.0;
    MISLAM_PLANE_UNROLL
    for (int j = 0; j < 6; j++) {
        double d = S[j][j];
        MISLAM_PLANE_UNROLL
        for (int k = 0; k < j; k++) d -= (S[j][k] * S[j][k]) * piv[k];
        piv[j] = d;
        if (!(d >= smallest)) smallest = d;                 // (a NaN pivot lands here too)
        if (!(d >= PLANE_PIVOT_MIN)) usable = false;
        MISLAM_PLANE_UNROLL
        for (int i = j + 1; i < 6; i++) {
            double s = S[i][j];
            MISLAM_PLANE_UNROLL
            for (int k = 0; k < j; k++) s -= (S[i][k] * S[j][k]) * piv[k];
            S[i][j] = s / d;
        }
    }
    if (min_pivot) *min_pivot = smallest;
    if (!usable) return false;
    double y[6];
    MISLAM_PLANE_UNROLL
    for (int i = 0; i < 6; i++) {                            // L z = -D^-1/2 g
        double s = -(g[i] * inv_root[i]);
        MISLAM_PLANE_UNROLL
        for (int k = 0; k < i; k++) s -= S[i][k] * y[k];
        y[i] = s;
    }
    MISLAM_PLANE_UNROLL
    for (int i = 0; i < 6; i++) y[i] = y[i] / piv[i];
    MISLAM_PLANE_UNROLL
    for (int i = 5; i >= 0; i--) {                           // L^T w = that
        double s = y[i];
        MISLAM_PLANE_UNROLL
        for (int k = i + 1; k < 6; k++) s -= S[k][i] * y[k];
        y[i] = s;
    }
    MISLAM_PLANE_UNROLL
    for (int i = 0; i < 6; i++) x[i] = y[i] * inv_root[i];
    return true;
}

MISLAM_PLANE_HD inline double plane_norm3(double x, double y, double z)
{
    using std::sqrt;
    return sqrt((x * x + y * y) + z * z);
}

MISLAM_PLANE_HD inline void plane_rodrigues(const double (&w)[3], double (&dR)[9])
{
    using std::sin;
    const double th2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2];
    const double th = plane_norm3(w[0], w[1], w[2]);
    double a, b;
    if (th < PLANE_SERIES_BELOW) {
        a = 1.0 - th2 / 6.0;
        b = 0.5 - th2 / 24.0;
    } else {
        const double sh = sin(0.5 * th);
        a = sin(th) / th;
        b = (2.0 * (sh * sh)) / th2;                        // 1 - cos(th) without its cancellation
    }
    // K = [omega]x, K^2 = omega omega^T - th^2 I
    dR[0] = 1.0 + b * (w[0] * w[0] - th2); dR[1] = b * (w[0] * w[1]) - a * w[2];  dR[2] = b * (w[0] * w[2]) + a * w[1];
    dR[3] = b * (w[0] * w[1]) + a * w[2];  dR[4] = 1.0 + b * (w[1] * w[1] - th2); dR[5] = b * (w[1] * w[2]) - a * w[0];
    dR[6] = b * (w[0] * w[2]) - a * w[1];  dR[7] = b * (w[1] * w[2]) + a * w[0];  dR[8] = 1.0 + b * (w[2] * w[2] - th2);
}

MISLAM_PLANE_HD inline void plane_compose(const double (&dR)[9], const double (&v)[3], const double (&c0)[3], double (&R)[9], double (&t)[3])
{
    double Rn[9];
    MISLAM_PLANE_UNROLL
    for (int i = 0; i < 3; i++) {
        MISLAM_PLANE_UNROLL
        for (int j = 0; j < 3; j++) Rn[3 * i + j] = (dR[3 * i] * R[j] + dR[3 * i + 1] * R[3 + j]) + dR[3 * i + 2] * R[6 + j];
    }
    const double d[3] = {t[0] - c0[0], t[1] - c0[1], t[2] - c0[2]};
    double tn[3];
    MISLAM_PLANE_UNROLL
    for (int i = 0; i < 3; i++) tn[i] = (((dR[3 * i] * d[0] + dR[3 * i + 1] * d[1]) + dR[3 * i + 2] * d[2]) + c0[i]) + v[i];
    MISLAM_PLANE_UNROLL
    for (int i = 0; i < 9; i++) R[i] = Rn[i];
    MISLAM_PLANE_UNROLL
    for (int i = 0; i < 3; i++) t[i] = tn[i];
}

}  // namespace mislam
