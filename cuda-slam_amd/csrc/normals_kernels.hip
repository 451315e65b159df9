// K14 -- surface normals and curvature of a cloud from every point's k nearest neighbours (mi_estimate_normals; driver: normals_api.hip).
//
// One launch does the search and the solve.  The search is K13's in self mode, the body of knn_scan.hpp: after it the lane holds its
// point's neighbourhood as K sorted keys in registers -- the same keys, bit for bit, that mi_knn_search would have written out.
//
//   moments  the keys are walked with static indices, predicated on "slot filled" (slot i belongs to the k-list, i >= K - k, and holds
//            a finite distance); the neighbour's coordinates come from the cloud's SoA in the caller's order, and the differences
//            d = p_j - p_i are taken in fp64, where two floats subtract exactly or round at 2^-53.  Nine fp64 sums: S = sum d, Q = sum d d^T,
//            added in the order of the keys (nearest first) -- a fixed order, so the same input gives the same bits.
//   matrix   with c = count + 1 points (the point itself contributes d = 0): m = S / c, C = Q / c - m m^T.  One pass is safe here because
//            every magnitude is bounded by the neighbourhood's radius r, not by the cloud's offset from the origin: |Q / c| and |m m^T| are
//            both <= r^2, against a covariance that is itself of the order r^2 in its largest direction; the cancellation costs a few 2^-53 of
//            the TRACE, which is all the smallest eigenvector's Rayleigh quotient is held to.
//   solve    eig3_symmetric (eig3.hpp): fp64 cyclic Jacobi in registers.  The normal is the eigenvector of the smallest eigenvalue, normalised
//            in fp64, turned towards the viewpoint if there is one (n . (v - p_i) >= 0, the test in fp64 on the unrounded vector), rounded
//            once to fp32.  Curvature = max(lambda0, 0) / (lambda0 + lambda1 + lambda2), 0 where that sum is not positive.
//   output   three floats to row order[s] of the caller's array, the curvature and the count where asked.  Fewer than three points
//            (count < 2): normal (0, 0, 0), curvature 0.  No LDS, no atomics, and the index lists never reach memory.
// mi_estimate_covariances (knn_covariances_kernel) is the same search and the same moments with the covariance itself as the output.
#include <hip/hip_runtime.h>

#include "eig3.hpp"
#include "kernels.h"
#include "knn_scan.hpp"
#include "nn_grid.h"

namespace mislam {

namespace {

// The search and the moments of one sorted slot, shared by the normals and the covariance kernel: K13's search in self mode, then the fp64
// one-pass covariance of the neighbourhood in the order of the keys.  Returns the neighbours found; cov (the upper triangle, row by row) is
// written where that is at least 2.
template <int K, bool FMA>
__device__ __forceinline__ int knn_neighbourhood_covariance(const NnGridView& g, const float (&q)[3], const float (&hi)[3], int row_out, int k, float max_d2,
                                                            const float* __restrict__ cx, const float* __restrict__ cy, const float* __restrict__ cz,
                                                            double (&cov)[6])
{
    unsigned long long l[K];
#pragma unroll
    for (int i = 0; i < K; i++) l[i] = i < K - k ? 0ull : KNN_KEY_EMPTY;
    knn_scan<K, FMA>(g, q, hi, (unsigned int)row_out, k, max_d2, l);

    const double qd[3] = {(double)q[0], (double)q[1], (double)q[2]};
    double sx = 0.0, sy = 0.0, sz = 0.0, qxx = 0.0, qxy = 0.0, qxz = 0.0, qyy = 0.0, qyz = 0.0, qzz = 0.0;
    int found = 0;
#pragma unroll
    for (int i = 0; i < K; i++) {
        if (i >= K - k && (unsigned int)(l[i] >> 32) < 0x7f800000u) {               // a filled slot of the k-list
            const unsigned int j = (unsigned int)(l[i] & 0xffffffffull);           // (< n: the index the grid build stored)
            const double dx = (double)cx[j] - qd[0], dy = (double)cy[j] - qd[1], dz = (double)cz[j] - qd[2];
            sx += dx; sy += dy; sz += dz;
            qxx += dx * dx; qxy += dx * dy; qxz += dx * dz;
            qyy += dy * dy; qyz += dy * dz; qzz += dz * dz;
            found++;
        }
    }
    if (found >= 2) {
        const double c = (double)(found + 1);
        const double mx = sx / c, my = sy / c, mz = sz / c;
        cov[0] = qxx / c - mx * mx; cov[1] = qxy / c - mx * my; cov[2] = qxz / c - mx * mz;
        cov[3] = qyy / c - my * my; cov[4] = qyz / c - my * mz; cov[5] = qzz / c - mz * mz;
    }
    return found;
}

// the unit eigenvector of cov's smallest eigenvalue, normalised in fp64
__device__ __forceinline__ void smallest_eigenvector(const double (&cov)[6], double (&lambda)[3], double& nx, double& ny, double& nz)
{
    double v[9];
    eig3_symmetric<double>(cov, lambda, v);
    nx = v[0]; ny = v[3]; nz = v[6];
    const double len = sqrt((nx * nx + ny * ny) + nz * nz);                       // (1 to rounding: V is a product of rotations)
    nx /= len; ny /= len; nz /= len;
}

template <int K, bool FMA>
__global__ __launch_bounds__(KNN_BLOCK) void knn_normals_kernel(NnGridView g, KnnNormalsArgs a)
{
    const int s = blockIdx.x * KNN_BLOCK + (int)threadIdx.x;
    if (s >= a.q.n) return;
    const float q[3] = {a.q.x[s], a.q.y[s], a.q.z[s]};     // (not knn_lane: through it this kernel takes one more SGPR at K = 8)
    const int row_out = a.q.order[s];

    double cov[6];
    const int found = knn_neighbourhood_covariance<K, FMA>(g, q, a.q.hi, row_out, a.k, a.max_d2, a.c.x, a.c.y, a.c.z, cov);

    double nx = 0.0, ny = 0.0, nz = 0.0, curv = 0.0;
    if (found >= 2) {
        const double qd[3] = {(double)q[0], (double)q[1], (double)q[2]};
        double lambda[3];
        smallest_eigenvector(cov, lambda, nx, ny, nz);
        if (a.oriented && (nx * (a.view[0] - qd[0]) + ny * (a.view[1] - qd[1])) + nz * (a.view[2] - qd[2]) < 0.0) { nx = -nx; ny = -ny; nz = -nz; }
        const double sum = (lambda[0] + lambda[1]) + lambda[2];
        curv = sum > 0.0 ? fmax(lambda[0], 0.0) / sum : 0.0;
    }
    float* out = a.normals + 3 * (size_t)row_out;
    out[0] = (float)nx; out[1] = (float)ny; out[2] = (float)nz;
    if (a.curvature) a.curvature[row_out] = (float)curv;
    if (a.count) a.count[row_out] = found;
}

// K17's covariance output (mi_estimate_covariances): the same neighbourhood and the same C; six floats per point instead of the normal.
//   raw    C rounded once to fp32 per entry
//   plane  I - (1 - epsilon) n n^T, n the fp64 unit eigenvector above: w = 1 - epsilon, u = w n (three products), entry ab = delta_ab - u_a n_b
//          (one product, one subtraction), rounded once.  The sign of n cancels in u_a n_b.
template <int K, bool FMA>
__global__ __launch_bounds__(KNN_BLOCK) void knn_covariances_kernel(NnGridView g, KnnCovariancesArgs a)
{
    const int s = blockIdx.x * KNN_BLOCK + (int)threadIdx.x;
    if (s >= a.n) return;
    const float q[3] = {a.qx[s], a.qy[s], a.qz[s]};
    const int row_out = a.order[s];

    double cov[6];
    const int found = knn_neighbourhood_covariance<K, FMA>(g, q, a.hi, row_out, a.k, a.max_d2, a.cx, a.cy, a.cz, cov);

    double c[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (found >= 2) {
        if (a.plane) {
            double lambda[3], nx, ny, nz;
            smallest_eigenvector(cov, lambda, nx, ny, nz);
            const double w = 1.0 - a.epsilon;
            const double ux = w * nx, uy = w * ny, uz = w * nz;
            c[0] = 1.0 - ux * nx; c[1] = 0.0 - ux * ny; c[2] = 0.0 - ux * nz;
            c[3] = 1.0 - uy * ny; c[4] = 0.0 - uy * nz; c[5] = 1.0 - uz * nz;
        } else {
#pragma unroll
            for (int i = 0; i < 6; i++) c[i] = cov[i];
        }
    }
    float* out = a.cov6 + 6 * (size_t)row_out;
#pragma unroll
    for (int i = 0; i < 6; i++) out[i] = (float)c[i];
    if (a.count) a.count[row_out] = found;
}

}  // namespace

hipError_t knn_normals(const NnGridView& g, const KnnNormalsArgs& a, int fma, hipStream_t s)
{
    if (a.q.n < 1 || a.k < 2 || a.k > KNN_MAX_K) return hipErrorInvalidValue;
    knn_dispatch(a.q.n, a.k, fma, [&](auto list, auto fused, dim3 grid) {
        hipLaunchKernelGGL((knn_normals_kernel<decltype(list)::value, decltype(fused)::value>), grid, dim3(KNN_BLOCK), 0, s, g, a);
    });
    return hipGetLastError();
}

hipError_t knn_covariances(const NnGridView& g, const KnnCovariancesArgs& a, int fma, hipStream_t s)
{
    if (a.n < 1 || a.k < 2 || a.k > KNN_MAX_K) return hipErrorInvalidValue;
    knn_dispatch(a.n, a.k, fma, [&](auto list, auto fused, dim3 grid) {
        hipLaunchKernelGGL((knn_covariances_kernel<decltype(list)::value, decltype(fused)::value>), grid, dim3(KNN_BLOCK), 0, s, g, a);
    });
    return hipGetLastError();
}

// loads this translation unit's code object at mi_ctx_preload (kernels.h)
__global__ void preload_normals_kernels_kernel() {}
hipError_t preload_normals_kernels()
{
    hipFuncAttributes attr;
    return hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(preload_normals_kernels_kernel));
}

}  // namespace mislam
