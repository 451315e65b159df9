// K50 -- moving-least-squares smoothing (mi_mls_smooth; driver: mls_api.hip).  The fixed-radius walk of K15's radius method (shell_walk,
// knn_scan.hpp) over ONE cell grid, one lane per query in the queries' curve order, twice, with a sink of its own each time.  Nothing is
// skipped: in self mode the query's own copy in the cloud is a point of its ball like any other.
//
//   first walk    K32's scatter about the query: a point with d2 <= r2 goes into nine fp64 running sums as the walk offers it, its coordinates
//                 from the cloud's SoA in the caller's order, d = p_j - q in fp64 (exact, or rounded at 2^-53), S += d, Q += d d^T.
//   between       a ball below min_neighbours leaves the query untouched and the lane does not walk again.  Otherwise mls_plane (mls_fit.hpp):
//                 the covariance, eig3_symmetric, the unit normal, the curvature, the query's foot on the plane and the frame.
//   second walk   ORDER == 2 and at least six points only: the same ball in the same order; the sink gathers the point again and mls_basis adds
//                 its row of the weighted normal equations to 21 + 6 fp64 sums.
//   behind        mls_project: plane_solve6 on the lane, the fall-back decision, the projection; then the stores to row order[s].
// The order of both sums is the walk's: shells outwards, rows of cells, the points of a cell as the grid build stored them -- a function of the
// cloud and the grid alone.  Everything lives in registers: every index into A, g and the plane's vectors is static once the loops of
// mls_fit.hpp are unrolled; no LDS, no atomics.  The registers and the scratch hipcc reports for gfx950: DESIGN.md section 4, K50.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "knn_scan.hpp"
#include "mls_fit.hpp"
#include "nn_grid.h"

namespace mislam {

namespace {

// the scatter of a ball about the query as a sink: the reach is r2, and a point AT r2 belongs (RadiusCountSink's rule without a skip)
struct MlsScatterSink {
    static constexpr bool LEAVES = false;
    float r2;
    const float *cx, *cy, *cz;
    double px, py, pz;
    double sx, sy, sz, qxx, qxy, qxz, qyy, qyz, qzz;
    int found;
    __device__ __forceinline__ bool take(float d2, unsigned int pj)
    {
        if (d2 <= r2) {                                                             // (pj < n: the index the grid build stored)
            const double dx = (double)cx[pj] - px, dy = (double)cy[pj] - py, dz = (double)cz[pj] - pz;
            sx += dx; sy += dy; sz += dz;
            qxx += dx * dx; qxy += dx * dy; qxz += dx * dz;
            qyy += dy * dy; qyz += dy * dz; qzz += dz * dz;
            found++;
        }
        return false;
    }
    __device__ __forceinline__ bool stop(float bound) const { return bound > r2; }
};

// the weighted normal equations of the quadratic over the plane as a sink: the same ball, the same order
struct MlsBasisSink {
    static constexpr bool LEAVES = false;
    float r2;
    const float *cx, *cy, *cz;
    double px, py, pz;
    double s2;
    const MlsPlane& plane;
    double (&A)[21];
    double (&g)[6];
    __device__ __forceinline__ bool take(float d2, unsigned int pj)
    {
        if (d2 <= r2) mls_basis(plane, (double)cx[pj] - px, (double)cy[pj] - py, (double)cz[pj] - pz, s2, A, g);
        return false;
    }
    __device__ __forceinline__ bool stop(float bound) const { return bound > r2; }
};

template <bool FMA, int ORDER>
__global__ __launch_bounds__(KNN_BLOCK) void mls_smooth_kernel(NnGridView g, MlsArgs a)
{
    float q[3];
    int row_out;
    if (!knn_lane(a.q, q, row_out)) return;
    const double qd[3] = {(double)q[0], (double)q[1], (double)q[2]};

    MlsScatterSink scatter{a.r2, a.c.x, a.c.y, a.c.z, qd[0], qd[1], qd[2], 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0};
    shell_walk<FMA>(g, q, a.q.hi, scatter);
    const int c = scatter.found;

    float xyz[3] = {q[0], q[1], q[2]}, normal[3] = {0.f, 0.f, 0.f}, curvature = 0.f;      // untouched: the query's input bits
    int status = MLS_UNTOUCHED;
    if (c >= a.min_neighbours) {                                                    // (>= 3, so c >= 1 below)
        const double S[3] = {scatter.sx, scatter.sy, scatter.sz};
        const double Q[6] = {scatter.qxx, scatter.qxy, scatter.qxz, scatter.qyy, scatter.qyz, scatter.qzz};
        MlsPlane plane;
        mls_plane(S, Q, c, plane);
        double A[21], rhs[6];
#pragma unroll
        for (int i = 0; i < 21; i++) A[i] = 0.0;
#pragma unroll
        for (int i = 0; i < 6; i++) rhs[i] = 0.0;
        if constexpr (ORDER == 2) {
            if (c >= MLS_QUADRATIC_MIN) {
                MlsBasisSink basis{a.r2, a.c.x, a.c.y, a.c.z, qd[0], qd[1], qd[2], a.s2, plane, A, rhs};
                shell_walk<FMA>(g, q, a.q.hi, basis);
            }
        }
        double x[3], m[3];
        status = mls_project(plane, qd, ORDER, c, A, rhs, x, m, nullptr);
#pragma unroll
        for (int k = 0; k < 3; k++) { xyz[k] = (float)x[k]; normal[k] = (float)m[k]; }
        curvature = (float)plane.curvature;
    }
    float* out = a.xyz + 3 * (size_t)row_out;
    out[0] = xyz[0]; out[1] = xyz[1]; out[2] = xyz[2];
    if (a.normals) {
        float* on = a.normals + 3 * (size_t)row_out;
        on[0] = normal[0]; on[1] = normal[1]; on[2] = normal[2];
    }
    if (a.curvature) a.curvature[row_out] = curvature;
    if (a.neighbours) a.neighbours[row_out] = c;
    if (a.status) a.status[row_out] = (unsigned char)status;
}

}  // namespace

hipError_t mls_smooth(const NnGridView& g, const MlsArgs& a, int order, int fma, hipStream_t s)
{
    if (a.q.n < 1 || a.min_neighbours < 3 || !(a.r2 >= 0.f) || !(a.s2 > 0.0) || (order != 1 && order != 2) || !a.xyz || !a.c.x || !a.c.y || !a.c.z)
        return hipErrorInvalidValue;
    const dim3 grid((a.q.n + KNN_BLOCK - 1) / KNN_BLOCK), block(KNN_BLOCK);
    if (order == 2) {
        if (fma) hipLaunchKernelGGL((mls_smooth_kernel<true, 2>), grid, block, 0, s, g, a);
        else hipLaunchKernelGGL((mls_smooth_kernel<false, 2>), grid, block, 0, s, g, a);
    } else {
        if (fma) hipLaunchKernelGGL((mls_smooth_kernel<true, 1>), grid, block, 0, s, g, a);
        else hipLaunchKernelGGL((mls_smooth_kernel<false, 1>), grid, block, 0, s, g, a);
    }
    return hipGetLastError();
}

// loads this translation unit's code object at mi_ctx_preload (kernels.h)
__global__ void preload_mls_kernels_kernel() {}
hipError_t preload_mls_kernels()
{
    hipFuncAttributes attr;
    return hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(preload_mls_kernels_kernel));
}

}  // namespace mislam
