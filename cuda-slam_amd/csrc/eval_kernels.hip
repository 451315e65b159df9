// K55 -- the quality of a pose on the device (mi_evaluate_registration; driver: eval_api.hip).  One launch of the step and K16's own rows
// reduce (plane_reduce_solve with solve = 0), nothing through the host:
//
//   step    the lane's move and row are pose_step.hpp's.  Its pair is the match of K16 (nearest_match: row i of mi_knn_search with k = 1), or,
//           GIVEN, the caller's pair_idx entry with the distance of the walk's own arithmetic (sq3 on the fp32 differences a_j - q); a
//           pair counts when its d2 is finite and within the limit.  The pair's numbers in fp64: a = a_j, d = q - a, and the three rows of
//           G = [-[a]x | I]; the row's entries are (G0i G0j + G1i G1j) + G2i G2j, (G0i d_x + G1i d_y) + G2i d_z and (d_x^2 + d_y^2) + d_z^2.
//           Most products of G's entries are 0 or 1 whatever the point: eval_lambda forms what is left, with the bits of the full expression
//           (the derivation stands beside it).
//   check   GIVEN: the lowest index of a pair_idx entry outside {-1} and [0, m), by an integer minimum.
// In both modes the lanes are the moving cloud's sorted slots, so the rows -- and with them every bit of the sums -- depend on the clouds
// and the pairs alone, not on where the pairs came from.  No float atomics anywhere.
#include <hip/hip_runtime.h>

#include <cmath>

#include "kernels.h"
#include "knn_scan.hpp"
#include "nn_grid.h"
#include "pose_step.hpp"
#include "reduce.hpp"

namespace mislam {

namespace {

// Entry (i, j), i <= j, of G^T G as the rule states it, (G0i G0j + G1i G1j) + G2i G2j with
//   G0 = (0, a_z, -a_y, 1, 0, 0)    G1 = (-a_z, 0, a_x, 0, 1, 0)    G2 = (a_y, -a_x, 0, 0, 0, 1),
// without the products that are zero whatever a is.  IEEE addition keeps x + (+0) = x except for x = -0, and the sum of two zeros of
// opposite signs is +0; with that, every entry below has the bits of the full expression for every finite a:
//   rotation block, diagonal       a square is never -0, so the product 0 * 0 = +0 beside two squares changes nothing
//   rotation block, off diagonal   the two zero products carry opposite signs (one has -a_k where the other has a_k): together +0, which
//                                  turns a product of -0 into +0 and leaves every other one as it is -- "0.0 + product"
//   rotation x translation         one entry of the column of -[a]x times 1 beside two zeros of which at least one is +0: "0.0 + entry";
//                                  on the block's diagonal that entry is the constant 0: +0
//   translation block              products of the constants 0 and 1: the identity
// one: 1.0 for a lane with a pair, 0.0 for one without (whose a is 0 too: all its entries are +0).
__device__ __forceinline__ double eval_lambda(int i, int j, double ax, double ay, double az, double one)
{
    switch (i * 6 + j) {
        case 0: return az * az + ay * ay;
        case 1: return 0.0 + ay * -ax;
        case 2: return 0.0 + -az * ax;
        case 4: return 0.0 + -az;
        case 5: return 0.0 + ay;
        case 7: return az * az + ax * ax;
        case 8: return 0.0 + az * -ay;
        case 9: return az + 0.0;
        case 11: return 0.0 + -ax;
        case 14: return ay * ay + ax * ax;
        case 15: return 0.0 + -ay;
        case 16: return 0.0 + ax;
        case 21: case 28: case 35: return one;
        default: return 0.0;                 // (0, 3), (1, 4), (2, 5) and the translation block off its diagonal
    }
}

template <bool FMA, bool GIVEN>
__global__ __launch_bounds__(KNN_BLOCK) void eval_step_kernel(NnGridView g, EvalStepArgs a)
{
    const PlaneState* __restrict__ st = a.state;
    const int lane = (int)threadIdx.x;
    const int s = blockIdx.x * KNN_BLOCK + lane;
    const bool live = s < a.q.n;

    double ax = 0.0, ay = 0.0, az = 0.0, dx = 0.0, dy = 0.0, dz = 0.0, d2d = 0.0, one = 0.0;
    if (live) {
        float q[3];
        pose_move(st, a.q.x[s], a.q.y[s], a.q.z[s], q);
        const int row = a.q.order[s];
        bool pair = false;
        unsigned int j = 0u, d2_bits = 0x7f800000u;
        if constexpr (GIVEN) {
            const int given = a.pair_idx[row];
            if (given >= 0 && given < a.m) {                                   // (the driver has refused anything else but -1)
                const float d2 = sq3<FMA>(a.c.x[given] - q[0], a.c.y[given] - q[1], a.c.z[given] - q[2]);
                if (d2 <= a.max_d2 && __float_as_uint(d2) < 0x7f800000u) { pair = true; j = (unsigned int)given; d2_bits = __float_as_uint(d2); }
            }
        } else {
            pair = nearest_match<FMA>(g, q, a.q.hi, a.max_d2, j, d2_bits);
        }
        if (pair) {
            ax = (double)a.c.x[j]; ay = (double)a.c.y[j]; az = (double)a.c.z[j];
            dx = (double)q[0] - ax; dy = (double)q[1] - ay; dz = (double)q[2] - az;
            d2d = (double)__uint_as_float(d2_bits);
            one = 1.0;
        }
        if (a.idx) a.idx[row] = pair ? (int)j : -1;
        if (a.d2) a.d2[row] = pair ? __uint_as_float(d2_bits) : INFINITY;
    }

    // g as the rule states it, the constants of G in their places (a lane without a pair holds d = a = 0: +0 everywhere)
    const double G0[6] = {0.0, az, -ay, 1.0, 0.0, 0.0}, G1[6] = {-az, 0.0, ax, 0.0, 1.0, 0.0}, G2[6] = {ay, -ax, 0.0, 0.0, 0.0, 1.0};
    pose_row_write(lane, a.rows + (size_t)blockIdx.x * PLANE_ROW, [&](int i, int j) { return eval_lambda(i, j, ax, ay, az, one); },
                   [&](int i) { return (G0[i] * dx + G1[i] * dy) + G2[i] * dz; }, (dx * dx + dy * dy) + dz * dz, d2d, one);
}

__global__ __launch_bounds__(256) void eval_check_pairs_kernel(const int* __restrict__ pair_idx, int n, int m, int* __restrict__ bad)
{
    const int i = blockIdx.x * 256 + (int)threadIdx.x;
    if (i >= n) return;
    const int v = pair_idx[i];
    if (v < -1 || v >= m) atomicMin(bad, i);
}

}  // namespace

hipError_t eval_step(const NnGridView& g, const EvalStepArgs& a, int fma, hipStream_t s)
{
    if (a.q.n < 1) return hipErrorInvalidValue;
    const dim3 grid(plane_row_count(a.q.n));
    const bool given = a.pair_idx != nullptr;
    if (given) {
        if (fma) hipLaunchKernelGGL((eval_step_kernel<true, true>), grid, dim3(KNN_BLOCK), 0, s, g, a);
        else hipLaunchKernelGGL((eval_step_kernel<false, true>), grid, dim3(KNN_BLOCK), 0, s, g, a);
    } else {
        if (fma) hipLaunchKernelGGL((eval_step_kernel<true, false>), grid, dim3(KNN_BLOCK), 0, s, g, a);
        else hipLaunchKernelGGL((eval_step_kernel<false, false>), grid, dim3(KNN_BLOCK), 0, s, g, a);
    }
    return hipGetLastError();
}

hipError_t eval_check_pairs(const int* pair_idx, int n, int m, int* bad, hipStream_t s)
{
    if (n < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(eval_check_pairs_kernel, dim3((n + 255) / 256), dim3(256), 0, s, pair_idx, n, m, bad);
    return hipGetLastError();
}

// loads this translation unit's code object at mi_ctx_preload (kernels.h)
__global__ void preload_eval_kernels_kernel() {}
hipError_t preload_eval_kernels()
{
    hipFuncAttributes attr;
    return hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(preload_eval_kernels_kernel));
}

}  // namespace mislam
