// K18 building block: the Darboux-frame features of one pair of oriented points and their bins, usable from one GPU lane and from host
// code (mi_fpfh_features, fpfh_kernels.hip; tests/fpfh_pair_selftest.cpp compiles this header alone with a host compiler).  The rules
// are those of include/mi_slam.h, operation for operation: every operand is a double, every operation is rounded (the build has
// -ffp-contract=off; a host build needs the same), sums of three are formed left to right, a cross-product component is two products
// and one subtraction.  Every value is a named scalar: no index is computed at run time, so the device code stays in registers.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MISLAM_FPFH_HD __host__ __device__
#else
#define MISLAM_FPFH_HD
#endif

#include <cmath>

namespace mislam {

constexpr int FPFH_BINS = 11;            // = MI_FPFH_BINS: bins per feature
constexpr int FPFH_DIM = 33;             // = MI_FPFH_DIM: theta's block, alpha's, phi's

// (theta, alpha, phi) of the pair (i, j): p the points, n the normals as given (neither checked for unit length nor normalised).
// (0, 0, 0) for a pair at distance 0 and for one whose d is parallel to u (or whose u is zero).
MISLAM_FPFH_HD inline void fpfh_pair_features(double pix, double piy, double piz, double nix, double niy, double niz, double pjx, double pjy,
                                              double pjz, double njx, double njy, double njz, double& theta, double& alpha, double& phi)
{
    using std::atan2;
    using std::fabs;
    using std::sqrt;
    theta = 0.0; alpha = 0.0; phi = 0.0;
    double dx = pjx - pix, dy = pjy - piy, dz = pjz - piz;
    const double len = sqrt((dx * dx + dy * dy) + dz * dz);
    if (len == 0.0) return;
    const double a1 = ((nix * dx + niy * dy) + niz * dz) / len;
    const double a2 = ((njx * dx + njy * dy) + njz * dz) / len;
    double ux, uy, uz, tx, ty, tz, f3;
    if (fabs(a1) < fabs(a2)) {           // the frame sits at the end whose normal is closer to the line between the points
        ux = njx; uy = njy; uz = njz; tx = nix; ty = niy; tz = niz;
        dx = -dx; dy = -dy; dz = -dz;
        f3 = -a2;
    } else {
        ux = nix; uy = niy; uz = niz; tx = njx; ty = njy; tz = njz;
        f3 = a1;
    }
    double vx = dy * uz - dz * uy, vy = dz * ux - dx * uz, vz = dx * uy - dy * ux;
    const double vl = sqrt((vx * vx + vy * vy) + vz * vz);
    if (vl == 0.0) return;
    vx = vx / vl; vy = vy / vl; vz = vz / vl;
    const double wx = uy * vz - uz * vy, wy = uz * vx - ux * vz, wz = ux * vy - uy * vx;
    alpha = (vx * tx + vy * ty) + vz * tz;
    theta = atan2((wx * tx + wy * ty) + wz * tz, (ux * tx + uy * ty) + uz * tz);
    phi = f3;
}

// floor(x) clamped to [0, 10]; a NaN goes to 0
MISLAM_FPFH_HD inline int fpfh_clamp_bin(double x)
{
    using std::floor;
    const double f = floor(x);
    return !(f >= 0.0) ? 0 : (f > 10.0 ? 10 : (int)f);
}

// the bin of theta within its block: [-pi, pi] in 11 equal parts
MISLAM_FPFH_HD inline int fpfh_bin_angle(double theta)
{
    const double pi = 3.141592653589793;
    return fpfh_clamp_bin((11.0 * (theta + pi)) / (2.0 * pi));
}

// the bin of alpha or phi within its block: [-1, 1] in 11 equal parts
MISLAM_FPFH_HD inline int fpfh_bin_cosine(double c) { return fpfh_clamp_bin((11.0 * (c + 1.0)) * 0.5); }

}  // namespace mislam
