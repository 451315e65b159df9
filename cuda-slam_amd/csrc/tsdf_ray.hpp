// The arithmetic of the TSDF map (mi_tsdf_integrate, mi_tsdf_extract, mi_slam.h), stated once for the device kernels (tsdf_kernels.hip), the
// host checks (tsdf_api.hip) and the CPU self-test (tests/tsdf_ray_selftest.cpp, which includes this header alone, without HIP): a ray from a
// posed point, its samples, a sample's voxel, the voxel's signed distance and value; a zero crossing between two voxels, its point, the
// gradient of the field at a voxel and the normal.  The move of a point is fp32 in the order of pose_step.hpp's pose_move; everything behind
// it is fp64 on promoted operands, every operation rounded once and none fused (every build has -ffp-contract=off), and only +, -, *, /,
// sqrt, floor and comparisons occur.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define MISLAM_TSDF_HD __host__ __device__ inline
#else
#define MISLAM_TSDF_HD inline
#endif

namespace mislam {

constexpr int TSDF_MAX_HALF_STEPS = 16;      // MI_TSDF_MAX_HALF_STEPS
constexpr float TSDF_MAX_ABS = 1e18f;        // a coordinate above this is refused

// kernels.h's voxel_axis in the same words (that header needs HIP; this one must not): floorf((p - o) / v), one IEEE subtraction and one
// IEEE division.  false: the quotient is not finite or outside [-2^30, 2^30).
MISLAM_TSDF_HD bool tsdf_voxel_axis(float p, float o, float v, int* out)
{
    const float q = floorf((p - o) / v);
    if (!(q >= -1073741824.f && q < 1073741824.f)) return false;
    *out = (int)q;
    return true;
}

// S, the half steps on either side of the hit: floor(truncation / (voxel_size / 2)) in fp64 (a caller refuses S > TSDF_MAX_HALF_STEPS)
MISLAM_TSDF_HD double tsdf_half_steps(float voxel, float truncation) { return floor((double)truncation / ((double)voxel / 2.0)); }

// w = ((R0 p_x + R1 p_y) + R2 p_z) + t, fp32, the expression of pose_move (pose_step.hpp) on a pose given as 16 floats, column-major
// (mi_icp_plane_register's out_T); T null: the identity, through the same expression.  o = the translation column.
MISLAM_TSDF_HD void tsdf_move(const float* T, float px, float py, float pz, float w[3], float o[3])
{
    for (int i = 0; i < 3; i++) {
        const float r0 = T ? T[i] : (i == 0 ? 1.f : 0.f), r1 = T ? T[4 + i] : (i == 1 ? 1.f : 0.f), r2 = T ? T[8 + i] : (i == 2 ? 1.f : 0.f);
        o[i] = T ? T[12 + i] : 0.f;
        w[i] = ((r0 * px + r1 * py) + r2 * pz) + o[i];
    }
}

struct TsdfRay {
    double o[3], w[3], d[3], rho;
};

// e = w - o, rho = sqrt((e_x^2 + e_y^2) + e_z^2), d = e / rho.  false: the ray contributes nothing (rho is 0, not finite, below min_range
// or above max_range).
MISLAM_TSDF_HD bool tsdf_ray(const float w[3], const float o[3], float min_range, float max_range, TsdfRay* r)
{
    double e[3];
    for (int i = 0; i < 3; i++) {
        r->o[i] = (double)o[i];
        r->w[i] = (double)w[i];
        e[i] = r->w[i] - r->o[i];
    }
    r->rho = sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]);
    if (!(r->rho > 0.0) || !(r->rho <= 1.7976931348623157e308)) return false;
    if (r->rho < (double)min_range || r->rho > (double)max_range) return false;
    for (int i = 0; i < 3; i++) r->d[i] = e[i] / r->rho;
    return true;
}

// Sample k of a ray.  0: s_k = rho + k h is not positive, the sample does not exist; -1: a voxel coordinate is outside [-2^30, 2^30);
// 1: c = the voxel of x_k = o + s_k d (one product and one sum per coordinate, rounded once to fp32).
MISLAM_TSDF_HD int tsdf_sample_voxel(const TsdfRay& r, int k, float voxel, const float origin[3], int c[3])
{
    const double h = (double)voxel / 2.0;
    const double s = r.rho + (double)k * h;
    if (!(s > 0.0)) return 0;
    for (int i = 0; i < 3; i++) {
        const float x = (float)(r.o[i] + s * r.d[i]);
        if (!tsdf_voxel_axis(x, origin[i], voxel, &c[i])) return -1;
    }
    return 1;
}

// the centre of voxel index c along one axis
MISLAM_TSDF_HD double tsdf_centre(int c, float origin, float voxel) { return (double)origin + ((double)c + 0.5) * (double)voxel; }

// The value of voxel c for a ray: sdf = (d_x (w_x - c_x) + d_y (w_y - c_y)) + d_z (w_z - c_z), positive on the sensor's side.  false: sdf is
// below -truncation, the voxel is behind the band.  Otherwise *f = min(1, sdf / truncation).
MISLAM_TSDF_HD bool tsdf_value(const TsdfRay& r, const int c[3], float voxel, const float origin[3], float truncation, double* f)
{
    const double tau = (double)truncation;
    const double t0 = r.d[0] * (r.w[0] - tsdf_centre(c[0], origin[0], voxel));
    const double t1 = r.d[1] * (r.w[1] - tsdf_centre(c[1], origin[1], voxel));
    const double t2 = r.d[2] * (r.w[2] - tsdf_centre(c[2], origin[2], voxel));
    const double sdf = (t0 + t1) + t2;
    if (sdf < -tau) return false;
    const double q = sdf / tau;
    *f = q < 1.0 ? q : 1.0;
    return true;
}

// The samples of a ray in ascending k, each surviving one handed to sink(k, c, f).  A sample whose voxel is that of sample k - 1 is
// dropped (sample k - 1 has a voxel when s_{k-1} > 0; the value depends on the voxel and the ray alone, so it does not matter whether
// k - 1 itself survived).  false: a sample's voxel coordinate was out of range; the walk stops there.
template <class Sink>
MISLAM_TSDF_HD bool tsdf_walk(const TsdfRay& r, int S, float voxel, const float origin[3], float truncation, Sink&& sink)
{
    bool have_prev = false;
    int p0 = 0, p1 = 0, p2 = 0;
    for (int k = -S; k <= S; k++) {
        int c[3];
        const int got = tsdf_sample_voxel(r, k, voxel, origin, c);
        if (got < 0) return false;
        if (got == 0) continue;
        const bool same = have_prev && c[0] == p0 && c[1] == p1 && c[2] == p2;
        have_prev = true; p0 = c[0]; p1 = c[1]; p2 = c[2];
        if (same) continue;
        double f;
        if (tsdf_value(r, c, voxel, origin, truncation, &f)) sink(k, c, f);
    }
    return true;
}

// ---- extraction
// Is there a zero crossing between a voxel of value f0 and its neighbour of value f1?  The signs differ (a value of exactly 0 counts as
// not positive) and not both values are saturated.  *r = f0 / (f0 - f1), in [0, 1] (a zero f0 gives -0, which moves nothing).
MISLAM_TSDF_HD bool tsdf_crossing(double f0, double f1, double* r)
{
    if ((f0 > 0.0) == (f1 > 0.0)) return false;
    if (fabs(f0) >= 1.0 && fabs(f1) >= 1.0) return false;
    *r = f0 / (f0 - f1);
    return true;
}

// the crossing's coordinate along its axis: the centre moved by r voxel_size, rounded once to fp32
MISLAM_TSDF_HD float tsdf_crossing_coord(int c, float origin, float voxel, double r) { return (float)(tsdf_centre(c, origin, voxel) + r * (double)voxel); }

// One axis of the field's gradient at a voxel of value f0, in voxels: the central difference where both neighbours are observed, the
// one-sided difference where one is, 0 where none is.
MISLAM_TSDF_HD double tsdf_gradient(bool has_minus, double f_minus, double f0, bool has_plus, double f_plus)
{
    if (has_minus && has_plus) return (f_plus - f_minus) / 2.0;
    if (has_plus) return f_plus - f0;
    if (has_minus) return f0 - f_minus;
    return 0.0;
}

// n = ((1 - r) g_i + r g_j) / its norm, rounded once to fp32; a zero (or non-finite) norm gives (0, 0, 0)
MISLAM_TSDF_HD void tsdf_normal(const double gi[3], const double gj[3], double r, float n[3])
{
    double v[3];
    for (int a = 0; a < 3; a++) v[a] = (1.0 - r) * gi[a] + r * gj[a];
    const double norm = sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
    for (int a = 0; a < 3; a++) n[a] = norm > 0.0 ? (float)(v[a] / norm) : 0.f;
}

// ---- the checks of a map as listed by a caller (host and self-test).  0: usable.  Otherwise the kind of the lowest refused row, and *row.
enum { TSDF_MAP_OK = 0, TSDF_MAP_COORD = 1, TSDF_MAP_ORDER = 2, TSDF_MAP_WEIGHT = 3, TSDF_MAP_VALUE = 4 };
MISLAM_TSDF_HD int tsdf_check_map(const int* coord, const float* tsdf, const float* weight, int nv, int* row, int cmin[3], int cmax[3])
{
    for (int i = 0; i < nv; i++) {
        const int* c = coord + 3 * (long long)i;
        *row = i;
        for (int a = 0; a < 3; a++)
            if (c[a] < -1073741824 || c[a] >= 1073741824) return TSDF_MAP_COORD;
        if (i > 0) {
            const int* p = c - 3;
            const bool above = c[2] != p[2] ? c[2] > p[2] : (c[1] != p[1] ? c[1] > p[1] : c[0] > p[0]);
            if (!above) return TSDF_MAP_ORDER;
        }
        if (!(weight[i] > 0.f) || !(weight[i] <= 3.4028234663852886e38f)) return TSDF_MAP_WEIGHT;
        if (!(tsdf[i] >= -1.f && tsdf[i] <= 1.f)) return TSDF_MAP_VALUE;
        for (int a = 0; a < 3; a++) {
            if (i == 0 || c[a] < cmin[a]) cmin[a] = c[a];
            if (i == 0 || c[a] > cmax[a]) cmax[a] = c[a];
        }
    }
    return TSDF_MAP_OK;
}

}  // namespace mislam
