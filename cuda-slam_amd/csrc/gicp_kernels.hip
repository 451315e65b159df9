// K17 -- generalized (plane-to-plane) ICP on the device (mi_icp_gicp_register, mi_gicp_system; driver: gicp_api.hip).  K16's iteration with a
// 3 x 3 information matrix per pair where K16 has a normal: the step kernel below writes K16's rows, and everything behind the rows -- the
// fixed-order sums, the 6 x 6 solve, the pose update, the stop rule, the state block -- is K16's own launch (plane_reduce_solve).
//
//   step    the lane's move, match and row are pose_step.hpp's.  Behind the match, every operand promoted to fp64 and every
//           operation rounded (-ffp-contract=off), with Rf the pose's rotation rounded to fp32 and C_b read at the lane's own slot:
//             T = Rf C_b              T_ic = (Rf_i0 Cb_0c + Rf_i1 Cb_1c) + Rf_i2 Cb_2c
//             Sigma = C_a + T Rf^T    S_ij = Ca_ij + ((T_i0 Rf_j0 + T_i1 Rf_j1) + T_i2 Rf_j2), i <= j
//             cofactors               c00 = S11 S22 - S12 S12   c01 = S02 S12 - S01 S22   c02 = S01 S12 - S02 S11
//                                     c11 = S00 S22 - S02 S02   c12 = S01 S02 - S00 S12   c22 = S00 S11 - S01 S01
//             det = (S00 c00 + S01 c01) + S02 c02;  a det that is <= 0 or not finite: no pair;  M_ij = c_ij / det
//           With d = q - a_j, P = q - c0 and (P x y)_0 = P_y y_2 - P_z y_1, (P x y)_1 = P_z y_0 - P_x y_2, (P x y)_2 = P_x y_1 - P_y y_0
//           (two products, one subtraction):
//             W = M J    W_ib = (P x M_i)_b for b < 3 (M_i: row i of M), M_i(b-3) beyond
//             H = J^T W  H_ab = (P x W_b)_a for a < 3 (W_b: column b of W), W_(a-3)b beyond; the 21 entries with a <= b
//             Md_i = (M_i0 d_x + M_i1 d_y) + M_i2 d_z;  g_a = (P x Md)_a for a < 3, Md_(a-3) beyond;  e = (d_x Md_0 + d_y Md_1) + d_z Md_2
//           The lane keeps P, M and d alive and hands the row its entries of H, g and e one at a time.
// No float atomics anywhere: the same input gives the same bits on every call.
#include <hip/hip_runtime.h>

#include <cfloat>

#include "gicp_terms.hpp"
#include "kernels.h"
#include "knn_scan.hpp"
#include "nn_grid.h"
#include "pose_step.hpp"
#include "reduce.hpp"

namespace mislam {

namespace {

template <bool FMA>
__global__ __launch_bounds__(KNN_BLOCK) __attribute__((amdgpu_waves_per_eu(8, 8))) void gicp_step_kernel(NnGridView g, GicpStepArgs a)
{
    const PlaneState* st = a.state;
    if (st->done != 0) return;
    const int lane = (int)threadIdx.x;
    const int s = blockIdx.x * KNN_BLOCK + lane;
    const bool live = s < a.q.n;

    bool pair = false;
    int match = -1;
    // (a lane without a pair holds zeros in M, P and d: its terms are +0)
    double M[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, P[3] = {0.0, 0.0, 0.0}, d[3] = {0.0, 0.0, 0.0}, d2d = 0.0;
    if (live) {
        float q[3];
        pose_move(st, a.q.x[s], a.q.y[s], a.q.z[s], q);
        unsigned int j, d2_bits;
        if (nearest_match<FMA>(g, q, a.q.hi, a.max_d2, j, d2_bits)) {
            __asm__ volatile("" ::: "memory");        // the pose is read again here (scalar loads) instead of living in VGPRs through the search
            const float Rf[9] = {(float)st->R[0], (float)st->R[1], (float)st->R[2], (float)st->R[3], (float)st->R[4], (float)st->R[5],
                                 (float)st->R[6], (float)st->R[7], (float)st->R[8]};
            const float4 a0 = a.cov_a[2 * (size_t)j], a1 = a.cov_a[2 * (size_t)j + 1];
            const float4 b0 = a.cov_b[2 * (size_t)s], b1 = a.cov_b[2 * (size_t)s + 1];
            const double Cb[6] = {(double)b0.x, (double)b0.y, (double)b0.z, (double)b1.x, (double)b1.y, (double)b1.z};
            const double Ca[6] = {(double)a0.x, (double)a0.y, (double)a0.z, (double)a1.x, (double)a1.y, (double)a1.z};
            double S[6];
#pragma unroll
            for (int i = 0; i < 3; i++) {
                const double r0 = (double)Rf[3 * i], r1 = (double)Rf[3 * i + 1], r2 = (double)Rf[3 * i + 2];
                const double T0 = (r0 * sym3(Cb, 0, 0) + r1 * sym3(Cb, 1, 0)) + r2 * sym3(Cb, 2, 0);
                const double T1 = (r0 * sym3(Cb, 0, 1) + r1 * sym3(Cb, 1, 1)) + r2 * sym3(Cb, 2, 1);
                const double T2 = (r0 * sym3(Cb, 0, 2) + r1 * sym3(Cb, 1, 2)) + r2 * sym3(Cb, 2, 2);
#pragma unroll
                for (int jj = i; jj < 3; jj++)
                    S[i == 0 ? jj : i + jj + 1] = sym3(Ca, i, jj) + ((T0 * (double)Rf[3 * jj] + T1 * (double)Rf[3 * jj + 1]) + T2 * (double)Rf[3 * jj + 2]);
            }
            const double c00 = S[3] * S[5] - S[4] * S[4], c01 = S[2] * S[4] - S[1] * S[5], c02 = S[1] * S[4] - S[2] * S[3];
            const double c11 = S[0] * S[5] - S[2] * S[2], c12 = S[1] * S[2] - S[0] * S[4], c22 = S[0] * S[3] - S[1] * S[1];
            const double det = (S[0] * c00 + S[1] * c01) + S[2] * c02;
            if (det > 0.0 && det <= DBL_MAX) {
                pair = true;
                match = (int)j;
                M[0] = c00 / det; M[1] = c01 / det; M[2] = c02 / det; M[3] = c11 / det; M[4] = c12 / det; M[5] = c22 / det;
                const double qx = (double)q[0], qy = (double)q[1], qz = (double)q[2];
                d[0] = qx - (double)a.c.x[j]; d[1] = qy - (double)a.c.y[j]; d[2] = qz - (double)a.c.z[j];
                P[0] = qx - st->c0[0]; P[1] = qy - st->c0[1]; P[2] = qz - st->c0[2];
                d2d = (double)__uint_as_float(d2_bits);
            }
        }
        if (a.idx) a.idx[a.q.order[s]] = match;
    }

    const double Md0 = (M[0] * d[0] + M[1] * d[1]) + M[2] * d[2];
    const double Md1 = (M[1] * d[0] + M[3] * d[1]) + M[4] * d[2];
    const double Md2 = (M[2] * d[0] + M[4] * d[1]) + M[5] * d[2];
    pose_row_write(
        lane, a.rows + (size_t)blockIdx.x * PLANE_ROW, [&](int i, int j) { return gicp_h(M, P, i, j); },
        [&](int i) { return i < 3 ? cross_at(P, i, Md0, Md1, Md2) : (i == 3 ? Md0 : (i == 4 ? Md1 : Md2)); }, (d[0] * Md0 + d[1] * Md1) + d[2] * Md2,
        d2d, pair ? 1.0 : 0.0);
}

__global__ __launch_bounds__(256) void gicp_pack_covariances_kernel(const float* __restrict__ cov6, int count, float4* __restrict__ packed, int* __restrict__ bad)
{
    const int i = blockIdx.x * 256 + (int)threadIdx.x;
    if (i >= count) return;
    const float* __restrict__ c = cov6 + 6 * (size_t)i;
    const float v[6] = {c[0], c[1], c[2], c[3], c[4], c[5]};
    bool usable = true;
#pragma unroll
    for (int e = 0; e < 6; e++) usable &= fabsf(v[e]) <= KNN_MAX_COORD;            // (false for NaN and the infinities)
    packed[2 * (size_t)i] = make_float4(v[0], v[1], v[2], 0.f);
    packed[2 * (size_t)i + 1] = make_float4(v[3], v[4], v[5], 0.f);
    if (!usable) atomicMin(bad, i);                                              // (an integer minimum: the same answer in any order)
}

__global__ __launch_bounds__(256) void gicp_permute_covariances_kernel(const float4* __restrict__ in, const int* __restrict__ order, int n, float4* __restrict__ out)
{
    const int s = blockIdx.x * 256 + (int)threadIdx.x;
    if (s >= n) return;
    const size_t from = 2 * (size_t)order[s];
    out[2 * (size_t)s] = in[from];
    out[2 * (size_t)s + 1] = in[from + 1];
}

}  // namespace

hipError_t gicp_step(const NnGridView& g, const GicpStepArgs& a, int fma, hipStream_t s)
{
    if (a.q.n < 1) return hipErrorInvalidValue;
    const dim3 grid(plane_row_count(a.q.n));
    if (fma) hipLaunchKernelGGL(gicp_step_kernel<true>, grid, dim3(KNN_BLOCK), 0, s, g, a);
    else hipLaunchKernelGGL(gicp_step_kernel<false>, grid, dim3(KNN_BLOCK), 0, s, g, a);
    return hipGetLastError();
}

hipError_t gicp_pack_covariances(const float* cov6, int count, float4* packed, int* bad, hipStream_t s)
{
    if (count < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(gicp_pack_covariances_kernel, dim3((count - 1) / 256 + 1), dim3(256), 0, s, cov6, count, packed, bad);
    return hipGetLastError();
}

hipError_t gicp_permute_covariances(const float4* in, const int* order, int n, float4* out, hipStream_t s)
{
    if (n < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(gicp_permute_covariances_kernel, dim3((n - 1) / 256 + 1), dim3(256), 0, s, in, order, n, out);
    return hipGetLastError();
}

// loads this translation unit's code object at mi_ctx_preload (kernels.h)
__global__ void preload_gicp_kernels_kernel() {}
hipError_t preload_gicp_kernels()
{
    hipFuncAttributes attr;
    return hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(preload_gicp_kernels_kernel));
}

}  // namespace mislam
