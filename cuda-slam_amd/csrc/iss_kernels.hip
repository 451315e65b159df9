// K32 / K33 -- ISS keypoints (mi_iss_keypoints; driver: iss_api.hip).  Both kernels are the fixed-radius walk of K15's radius method
// (shell_walk, knn_scan.hpp) over ONE cell grid, one lane per point in curve order, with a sink of their own in the place of its counter.
//
//   K32 saliency   the sink takes a point of the salient ball (j != self by index, d2 <= r2s) into nine fp64 running sums as the walk
//                  offers it: the neighbour's coordinates come from the cloud's SoA in the caller's order, d = p_j - p_i in fp64 (exact,
//                  or rounded at 2^-53), S += d, Q += d d^T (upper triangle), one product and one addition per entry.  The order is the
//                  walk's: shells outwards, rows of cells, the points of a cell run as the grid build stored them -- a function of the
//                  cloud and the grid alone.  Behind the walk, K14's matrix rule with c = count + 1: m = S / c, C = Q / c - m m^T, then
//                  eig3_symmetric<double> (its V is dead code here), the gate by products and the saliency, all to row order[s].
//                  Everything is a named scalar in registers: no LDS, no scratch, no run-time index into an array.
//   K33 suppress   a lane whose saliency is 0 writes 0 and does not walk.  A candidate walks its non-max ball (d2 <= r2n), counts it,
//                  gathers saliency[j] by caller index and leaves the walk at the first j that dominates it: saliency[j] > saliency[i], or
//                  equal and j < i.  A keypoint has walked its whole ball, found no such j and counted at least min_neighbours.
// The flags go through K15's compaction (outlier_compact).  No atomics anywhere.
#include <hip/hip_runtime.h>

#include "eig3.hpp"
#include "kernels.h"
#include "knn_scan.hpp"
#include "nn_grid.h"

namespace mislam {

namespace {

// the scatter of a ball as a sink: the reach is r2, and a point AT r2 belongs (RadiusCountSink's rule, so `found` is its count)
struct IssScatterSink {
    static constexpr bool LEAVES = false;
    unsigned int skip;
    float r2;
    const float *cx, *cy, *cz;
    double px, py, pz;
    double sx, sy, sz, qxx, qxy, qxz, qyy, qyz, qzz;
    int found;
    __device__ __forceinline__ bool take(float d2, unsigned int pj)
    {
        if (pj != skip && d2 <= r2) {                                               // (pj < n: the index the grid build stored)
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

// the non-max ball as a sink: counts it, and leaves at the first neighbour that dominates `mine`
struct IssDominanceSink {
    static constexpr bool LEAVES = true;
    unsigned int self;
    float r2;
    const float* saliency;
    float mine;
    int found;
    bool dominated;
    __device__ __forceinline__ bool take(float d2, unsigned int pj)
    {
        if (pj != self && d2 <= r2) {
            found++;
            const float other = saliency[pj];                                       // (pj < n, as above)
            if (other > mine || (other == mine && pj < self)) {
                dominated = true;
                return true;
            }
        }
        return false;
    }
    __device__ __forceinline__ bool stop(float bound) const { return bound > r2; }
};

template <bool FMA>
__global__ __launch_bounds__(KNN_BLOCK) void iss_saliency_kernel(NnGridView g, IssSaliencyArgs a)
{
    float q[3];
    int row_out;
    if (!knn_lane(a.q, q, row_out)) return;

    IssScatterSink sink{(unsigned int)row_out, a.r2, a.c.x, a.c.y, a.c.z, (double)q[0], (double)q[1], (double)q[2],
                        0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0};
    shell_walk<FMA>(g, q, a.q.hi, sink);

    const double c = (double)(sink.found + 1);                                      // the point itself contributes d = 0
    const double mx = sink.sx / c, my = sink.sy / c, mz = sink.sz / c;
    const double cov[6] = {sink.qxx / c - mx * mx, sink.qxy / c - mx * my, sink.qxz / c - mx * mz,
                           sink.qyy / c - my * my, sink.qyz / c - my * mz, sink.qzz / c - mz * mz};
    double lambda[3], v[9];
    eig3_symmetric<double>(cov, lambda, v);                                         // (an empty ball: the zero matrix, lambda = 0)

    const bool gate = sink.found >= a.min_neighbours && lambda[1] < a.gamma_21 * lambda[2] && lambda[0] < a.gamma_32 * lambda[1];
    const float l0 = (float)lambda[0];
    a.saliency[row_out] = gate && l0 > 0.f ? l0 : 0.f;
    if (a.eigenvalues) {
        float* out = a.eigenvalues + 3 * (size_t)row_out;
        out[0] = l0; out[1] = (float)lambda[1]; out[2] = (float)lambda[2];
    }
    if (a.neighbours) a.neighbours[row_out] = sink.found;
}

template <bool FMA>
__global__ __launch_bounds__(KNN_BLOCK) void iss_suppress_kernel(NnGridView g, IssSuppressArgs a)
{
    float q[3];
    int row_out;
    if (!knn_lane(a.q, q, row_out)) return;
    const float mine = a.saliency[row_out];
    unsigned char flag = 0;
    if (mine > 0.f) {
        IssDominanceSink sink{(unsigned int)row_out, a.r2, a.saliency, mine, 0, false};
        shell_walk<FMA>(g, q, a.q.hi, sink);
        flag = !sink.dominated && sink.found >= a.min_neighbours ? 1 : 0;
    }
    a.is_keypoint[row_out] = flag;
}

}  // namespace

hipError_t iss_saliency(const NnGridView& g, const IssSaliencyArgs& a, int fma, hipStream_t s)
{
    if (a.q.n < 1 || a.min_neighbours < 1 || !(a.r2 >= 0.f) || !a.saliency || !a.c.x || !a.c.y || !a.c.z) return hipErrorInvalidValue;
    const dim3 grid((a.q.n + KNN_BLOCK - 1) / KNN_BLOCK), block(KNN_BLOCK);
    if (fma) hipLaunchKernelGGL((iss_saliency_kernel<true>), grid, block, 0, s, g, a);
    else hipLaunchKernelGGL((iss_saliency_kernel<false>), grid, block, 0, s, g, a);
    return hipGetLastError();
}

hipError_t iss_suppress(const NnGridView& g, const IssSuppressArgs& a, int fma, hipStream_t s)
{
    if (a.q.n < 1 || a.min_neighbours < 1 || !(a.r2 >= 0.f) || !a.saliency || !a.is_keypoint) return hipErrorInvalidValue;
    const dim3 grid((a.q.n + KNN_BLOCK - 1) / KNN_BLOCK), block(KNN_BLOCK);
    if (fma) hipLaunchKernelGGL((iss_suppress_kernel<true>), grid, block, 0, s, g, a);
    else hipLaunchKernelGGL((iss_suppress_kernel<false>), grid, block, 0, s, g, a);
    return hipGetLastError();
}

// loads this translation unit's code object at mi_ctx_preload (kernels.h)
__global__ void preload_iss_kernels_kernel() {}
hipError_t preload_iss_kernels()
{
    hipFuncAttributes attr;
    return hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(preload_iss_kernels_kernel));
}

}  // namespace mislam
