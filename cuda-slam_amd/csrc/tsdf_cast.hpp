// The arithmetic of mi_tsdf_raycast (mi_slam.h), stated once for the device kernel (tsdf_kernels.hip, K75), the host checks (tsdf_api.hip) and
// the CPU self-test (tests/tsdf_cast_selftest.cpp, which includes this header and tsdf_ray.hpp alone, without HIP): a ray from a direction in
// the sensor's frame, its samples and their voxels, the march to the first sign change seen from the positive side, the trilinear field, the
// hit's depth, point and normal.  The rotation of the direction is fp32; everything behind it is fp64 on promoted operands, every operation
// rounded once and none fused (every build has -ffp-contract=off), and only +, -, *, /, sqrt, floor and comparisons occur.  The map is reached
// through two callables, so the same words run over the device's tables and over a host container:
//   lookup(cx, cy, cz)    the row of the OBSERVED voxel (cx, cy, cz), or -1;
//   occupied(bx, by, bz)  does the block (bx, by, bz) of 8^3 voxels (block = voxel coordinate >> 3), or one of its 26 neighbours, hold an
//                         observed voxel?  Asked only while skipping is on.
#pragma once
#include "tsdf_ray.hpp"

#if defined(__HIPCC__)
#define MISLAM_TSDF_UNROLL _Pragma("unroll")
#else
#define MISLAM_TSDF_UNROLL
#endif

namespace mislam {

constexpr int TSDF_RAYCAST_MAX_STEPS = 65536;        // MI_TSDF_RAYCAST_MAX_STEPS
constexpr int TSDF_SKIP_SHIFT = 3;                   // a block of the coarse table is 8 voxels along each axis
// Empty-space skipping ("TSDF ray casting", has the proof).  A sample whose voxel c lies in an unoccupied block has no observed
// voxel within 8 voxels of c along any axis (Chebyshev distance <= 8: the nearest voxel of a block two blocks away is 9 away).  Two samples j
// steps apart lie j / 2 voxels apart at the most; their voxels are found from positions rounded to fp32 by two fp32 operations, which moves
// each sample's real voxel coordinate by E <= 2^-24 (|x| + 2 |x - origin|) / voxel_size at the most, and floor adds less than 1.  So the voxels
// differ by less than j / 2 + 2 E + 1, and with j <= 14 and E <= 1 / 4 by less than 9: the 14 samples behind such a sample are unobserved and
// the march may step over them.  tsdf_cast_skip_sound bounds E by 1 / 8 over the whole ray; where it does not hold the driver marches plainly.
constexpr int TSDF_SKIP_SAMPLES = 14;
constexpr double TSDF_SKIP_LIMIT = 2097152.0;        // 2^21: (3 max|o| + 2 max|origin| + 3 max_range) / voxel_size at the most

// K = floor((max_range - min_range) / (voxel_size / 2)) + 1 in fp64 (a caller refuses K > TSDF_RAYCAST_MAX_STEPS)
MISLAM_TSDF_HD double tsdf_cast_steps(float voxel, float min_range, float max_range)
{
    return floor(((double)max_range - (double)min_range) / ((double)voxel / 2.0)) + 1.0;
}

// Is the skip sound for every ray of a call?  |x| <= max|o| + max_range and |x - origin| <= max|o| + max|origin| + max_range along every axis of
// every sample, so E <= 2^-24 (3 max|o| + 2 max|origin| + 3 max_range) / voxel_size <= 2^-24 2^21 = 1 / 8.
MISLAM_TSDF_HD bool tsdf_cast_skip_sound(const float* T, const float origin[3], float voxel, float max_range)
{
    double o = 0.0, g = 0.0;
    for (int a = 0; a < 3; a++) {
        const double oa = fabs(T ? (double)T[12 + a] : 0.0), ga = fabs((double)origin[a]);
        if (oa > o) o = oa;
        if (ga > g) g = ga;
    }
    return (3.0 * o + 2.0 * g + 3.0 * (double)max_range) / (double)voxel <= TSDF_SKIP_LIMIT;
}

struct TsdfCastRay {
    double o[3], d[3];
};

// o = T's translation column; u = (R0 d_x + R1 d_y) + R2 d_z per row of R in fp32, tsdf_move's expression without the translation (T null:
// the identity through the same expression); len = sqrt((u_x^2 + u_y^2) + u_z^2) and d = u / len in fp64.  false: len is 0 or not finite, the
// ray is a miss.
MISLAM_TSDF_HD bool tsdf_cast_dir(const float* T, float dx, float dy, float dz, TsdfCastRay* r)
{
    double u[3];
    for (int i = 0; i < 3; i++) {
        const float r0 = T ? T[i] : (i == 0 ? 1.f : 0.f), r1 = T ? T[4 + i] : (i == 1 ? 1.f : 0.f), r2 = T ? T[8 + i] : (i == 2 ? 1.f : 0.f);
        r->o[i] = T ? (double)T[12 + i] : 0.0;
        u[i] = (double)((r0 * dx + r1 * dy) + r2 * dz);
    }
    const double len = sqrt((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]);
    if (!(len > 0.0) || !(len <= 1.7976931348623157e308)) return false;
    for (int i = 0; i < 3; i++) r->d[i] = u[i] / len;
    return true;
}

struct TsdfCastGeom {
    float origin[3], voxel, min_range;
    int steps;                           // K
};

// s_k = min_range + k h, one product and one sum
MISLAM_TSDF_HD double tsdf_cast_depth(const TsdfCastGeom& g, int k) { return (double)g.min_range + (double)k * ((double)g.voxel / 2.0); }

// The voxel of sample k: x_k = o + s_k d per coordinate, rounded once to fp32, placed as mi_voxel_index places it.  false: a voxel coordinate
// is outside [-2^30, 2^30), the sample is unobserved.
MISLAM_TSDF_HD bool tsdf_cast_sample_voxel(const TsdfCastRay& r, const TsdfCastGeom& g, int k, int c[3])
{
    const double s = tsdf_cast_depth(g, k);
    for (int i = 0; i < 3; i++) {
        const float x = (float)(r.o[i] + s * r.d[i]);
        if (!tsdf_voxel_axis(x, g.origin[i], g.voxel, &c[i])) return false;
    }
    return true;
}

// The trilinear field at depth s.  false: not available -- one of the eight corner voxels is unobserved, or a corner index is outside
// [-2^30, 2^30).  At most 8 look-ups.
template <class Lookup>
MISLAM_TSDF_HD bool tsdf_cast_field(const TsdfCastRay& r, const TsdfCastGeom& g, double s, const float* tsdf, Lookup&& lookup, double* F)
{
    int i[3];
    double w[3];
    for (int a = 0; a < 3; a++) {
        const double p = r.o[a] + s * r.d[a];
        const double q = (p - (double)g.origin[a]) / (double)g.voxel - 0.5;
        if (!(q >= -1073741824.0 && q < 1073741824.0)) return false;
        const double fl = floor(q);
        i[a] = (int)fl;
        w[a] = q - fl;
    }
    double c[2][2];                      // c_yz
MISLAM_TSDF_UNROLL
    for (int z = 0; z < 2; z++)
MISLAM_TSDF_UNROLL
        for (int y = 0; y < 2; y++) {
            const int r0 = lookup(i[0], i[1] + y, i[2] + z);
            if (r0 < 0) return false;
            const int r1 = lookup(i[0] + 1, i[1] + y, i[2] + z);
            if (r1 < 0) return false;
            const double f0 = (double)tsdf[r0], f1 = (double)tsdf[r1];
            c[y][z] = f0 + w[0] * (f1 - f0);
        }
    const double c0 = c[0][0] + w[1] * (c[1][0] - c[0][0]), c1 = c[0][1] + w[1] * (c[1][1] - c[0][1]);
    *F = c0 + w[2] * (c1 - c0);
    return true;
}

// the gradient of the field at the observed voxel c of value f over its observed neighbours, as the extraction takes it: 6 look-ups
template <class Lookup>
MISLAM_TSDF_HD void tsdf_cast_gradient(const int c[3], double f, const float* tsdf, Lookup&& lookup, double g[3])
{
MISLAM_TSDF_UNROLL
    for (int ax = 0; ax < 3; ax++) {
        const int dx = ax == 0, dy = ax == 1, dz = ax == 2;
        const int m = lookup(c[0] - dx, c[1] - dy, c[2] - dz), p = lookup(c[0] + dx, c[1] + dy, c[2] + dz);
        g[ax] = tsdf_gradient(m >= 0, m >= 0 ? (double)tsdf[m] : 0.0, f, p >= 0, p >= 0 ? (double)tsdf[p] : 0.0);
    }
}

struct TsdfCastHit {
    float depth, xyz[3], normal[3];
    int k;                               // the sample the march ended at (steps: it ran out); what follows is set for a hit alone
    int trilinear;                       // 1: r came from the trilinear field, 0: from the two voxels' values
    double r;
};

// One ray: the march of rule 3 over k ascending, one look-up per visited sample, and for a hit rules 4 and 5, 16 + 12 look-ups at the most.
// false: a miss, *out all zero but for k.  skip: leave out the samples tsdf_cast_skip_sound lets the march prove unobserved; it moves no bit.
template <class Lookup, class Occupied>
MISLAM_TSDF_HD bool tsdf_cast(const TsdfCastRay& r, const TsdfCastGeom& g, const float* tsdf, Lookup&& lookup, bool skip, Occupied&& occupied, TsdfCastHit* out)
{
    out->depth = 0.f;
    for (int a = 0; a < 3; a++) out->xyz[a] = out->normal[a] = 0.f;
    out->k = g.steps; out->trilinear = 0; out->r = 0.0;
    bool prev_observed = false, have_block = false;
    double prev_g = 0.0;
    int pc[3] = {0, 0, 0}, ob[3] = {0, 0, 0};            // the voxel of sample k - 1; the block last found occupied
    for (int k = 0; k < g.steps; k++) {
        int c[3];
        if (!tsdf_cast_sample_voxel(r, g, k, c)) { prev_observed = false; continue; }
        const int row = lookup(c[0], c[1], c[2]);
        if (row < 0) {
            prev_observed = false;
            if (skip) {
                const int b0 = c[0] >> TSDF_SKIP_SHIFT, b1 = c[1] >> TSDF_SKIP_SHIFT, b2 = c[2] >> TSDF_SKIP_SHIFT;   // (arithmetic shifts: floor)
                if (!(have_block && b0 == ob[0] && b1 == ob[1] && b2 == ob[2])) {
                    if (occupied(b0, b1, b2)) { have_block = true; ob[0] = b0; ob[1] = b1; ob[2] = b2; }
                    else k += TSDF_SKIP_SAMPLES;         // samples k + 1 .. k + 14 are unobserved: sample k + 15 is the next one visited
                }
            }
            continue;
        }
        const double gk = (double)tsdf[row];
        if (gk > 0.0) {
            prev_observed = true; prev_g = gk;
            pc[0] = c[0]; pc[1] = c[1]; pc[2] = c[2];
            continue;
        }
        out->k = k;
        if (k < 1 || !prev_observed) return false;       // met from behind or from unobserved space
        const double h = (double)g.voxel / 2.0, a = tsdf_cast_depth(g, k - 1), b = tsdf_cast_depth(g, k);
        double Fa = 0.0, Fb = 0.0;
        const bool tri = tsdf_cast_field(r, g, a, tsdf, lookup, &Fa) && tsdf_cast_field(r, g, b, tsdf, lookup, &Fb) && Fa > 0.0 && 0.0 >= Fb;
        const double ratio = tri ? Fa / (Fa - Fb) : prev_g / (prev_g - gk);
        const double t = a + ratio * h;
        const float depth = (float)t;
        if (!(depth > 0.f)) return false;                // (a depth that rounds to 0 in fp32: the depth is the hit flag, so this is a miss)
        out->depth = depth;
        for (int i = 0; i < 3; i++) out->xyz[i] = (float)(r.o[i] + t * r.d[i]);
        double gi[3], gj[3];
        tsdf_cast_gradient(pc, prev_g, tsdf, lookup, gi);
        tsdf_cast_gradient(c, gk, tsdf, lookup, gj);
        tsdf_normal(gi, gj, ratio, out->normal);
        out->trilinear = tri ? 1 : 0;
        out->r = ratio;
        return true;
    }
    return false;
}

}  // namespace mislam
