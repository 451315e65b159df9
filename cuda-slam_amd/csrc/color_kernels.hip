// K48 / K49 -- colored ICP on the device (mi_estimate_color_gradients, mi_icp_color_register, mi_color_system; driver: color_api.hip; the
// arithmetic of a point's gradient and of a pair: color_terms.hpp).
//
//   K48 gradient  K14's shape: K13's search in self mode (knn_scan.hpp), after which the lane holds its point's neighbourhood as K sorted
//                 keys in registers -- the keys mi_knn_search would have written out, bit for bit.  The keys are walked with static
//                 indices, nearest first; per filled slot the neighbour's offset e = p_j - p_i and intensity step I_j - I_i are taken in
//                 fp64 and added to the nine sums of the tangent-plane least squares (color_gradient_add).  Behind the walk the
//                 constraint d . n = 0 and the 3 x 3 solve by the adjugate run in the lane (color_gradient_constrain, color_gradient_solve);
//                 three floats go to row order[s] of the caller's array.  No LDS, no atomics, and the index lists never reach memory.
//   K49 step      K16's step with a second residual: the lane's move, match and row are pose_step.hpp's; behind the match the pair's
//                 geometric and photometric Jacobian rows and residuals (color_pair_terms) stay alive in the lane, and the row's entries
//                 are their weighted products, one at a time.  It writes K16's rows, so the reduce, the solve, the state block and the
//                 rules are K16's own launch (plane_reduce_solve).
// The small kernels behind them check and repack what the caller brought beside the clouds: intensities and gradients.
// No float atomics anywhere: the same input gives the same bits on every call.
#include <hip/hip_runtime.h>

#include "color_terms.hpp"
#include "kernels.h"
#include "knn_scan.hpp"
#include "nn_grid.h"
#include "pose_step.hpp"
#include "reduce.hpp"

namespace mislam {

namespace {

template <int K, bool FMA>
__global__ __launch_bounds__(KNN_BLOCK) void color_gradient_kernel(NnGridView g, ColorGradientArgs a)
{
    const int s = blockIdx.x * KNN_BLOCK + (int)threadIdx.x;
    if (s >= a.q.n) return;
    const float q[3] = {a.q.x[s], a.q.y[s], a.q.z[s]};
    const int row_out = a.q.order[s];

    unsigned long long l[K];
#pragma unroll
    for (int i = 0; i < K; i++) l[i] = i < K - a.k ? 0ull : KNN_KEY_EMPTY;
    knn_scan<K, FMA>(g, q, a.q.hi, (unsigned int)row_out, a.k, a.max_d2, l);

    const double qd[3] = {(double)q[0], (double)q[1], (double)q[2]};
    const double n[3] = {(double)a.nx[row_out], (double)a.ny[row_out], (double)a.nz[row_out]};
    const double Ii = (double)a.intensity[row_out];
    double M[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, b[3] = {0.0, 0.0, 0.0};
    int found = 0;
#pragma unroll
    for (int i = 0; i < K; i++) {
        if (i >= K - a.k && (unsigned int)(l[i] >> 32) < 0x7f800000u) {               // a filled slot of the k-list
            const unsigned int j = (unsigned int)(l[i] & 0xffffffffull);           // (< n: the index the grid build stored)
            color_gradient_add(n, (double)a.c.x[j] - qd[0], (double)a.c.y[j] - qd[1], (double)a.c.z[j] - qd[2], (double)a.intensity[j] - Ii, M, b);
            found++;
        }
    }
    double d[3] = {0.0, 0.0, 0.0};
    if (found >= 2 && (n[0] != 0.0 || n[1] != 0.0 || n[2] != 0.0)) {
        color_gradient_constrain(n, found, M);
        color_gradient_solve(M, b, d);
    }
    float* out = a.gradients + 3 * (size_t)row_out;
    out[0] = (float)d[0]; out[1] = (float)d[1]; out[2] = (float)d[2];
    if (a.count) a.count[row_out] = found;
}

template <bool FMA>
__global__ __launch_bounds__(KNN_BLOCK) void color_step_kernel(NnGridView g, ColorStepArgs a)
{
    const PlaneState* __restrict__ st = a.state;
    if (st->done != 0) return;
    const int lane = (int)threadIdx.x;
    const int s = blockIdx.x * KNN_BLOCK + lane;
    const bool live = s < a.q.n;

    bool pair = false;
    int match = -1;
    ColorPair p;
    color_pair_none(p);
    double d2d = 0.0;
    if (live) {
        float q[3];
        pose_move(st, a.q.x[s], a.q.y[s], a.q.z[s], q);
        unsigned int j, d2_bits;
        if (nearest_match<FMA>(g, q, a.q.hi, a.max_d2, j, d2_bits)) {
            const float4 nf = a.normals[j];
            if (nf.x != 0.f || nf.y != 0.f || nf.z != 0.f) {
                pair = true;
                match = (int)j;
                const float4 gi = a.grad_i[j];
                const double qd[3] = {(double)q[0], (double)q[1], (double)q[2]};
                const double ad[3] = {(double)a.c.x[j], (double)a.c.y[j], (double)a.c.z[j]};
                const double c0[3] = {st->c0[0], st->c0[1], st->c0[2]};
                const double nd[3] = {(double)nf.x, (double)nf.y, (double)nf.z};
                const double gd[3] = {(double)gi.x, (double)gi.y, (double)gi.z};
                color_pair_terms(qd, ad, c0, nd, gd, (double)gi.w, (double)a.ib[s], p);
                d2d = (double)__uint_as_float(d2_bits);
            }
        }
        if (a.idx) a.idx[a.q.order[s]] = match;
    }

    const double lg = a.lambda, lc = 1.0 - lg;
    pose_row_write(lane, a.rows + (size_t)blockIdx.x * PLANE_ROW, [&](int i, int j) { return color_pair_h(p, lg, lc, i, j); },
                   [&](int i) { return color_pair_g(p, lg, lc, i); }, color_pair_e(p, lg, lc), d2d, pair ? 1.0 : 0.0);
}

// *bad = min(*bad, the lowest index with a value that is not finite or above 1e18 in magnitude) -- the caller sets *bad to KNN_NO_POINT first
__global__ __launch_bounds__(256) void color_check_values_kernel(const float* __restrict__ v, int count, int* __restrict__ bad)
{
    const int i = blockIdx.x * 256 + (int)threadIdx.x;
    if (i >= count) return;
    if (!(fabsf(v[i]) <= KNN_MAX_COORD)) atomicMin(bad, i);                        // (an integer minimum: the same answer in any order)
}

__global__ __launch_bounds__(256) void color_pack_fixed_kernel(const float* __restrict__ grad3, const float* __restrict__ intensity, int m,
                                                               float4* __restrict__ packed, int* __restrict__ bad_intensity, int* __restrict__ bad_gradient)
{
    const int i = blockIdx.x * 256 + (int)threadIdx.x;
    if (i >= m) return;
    const float* __restrict__ gp = grad3 + 3 * (size_t)i;
    const float gx = gp[0], gy = gp[1], gz = gp[2], I = intensity[i];
    packed[i] = make_float4(gx, gy, gz, I);
    if (!(fabsf(I) <= KNN_MAX_COORD)) atomicMin(bad_intensity, i);
    if (!(fabsf(gx) <= KNN_MAX_COORD && fabsf(gy) <= KNN_MAX_COORD && fabsf(gz) <= KNN_MAX_COORD)) atomicMin(bad_gradient, i);
}

__global__ __launch_bounds__(256) void color_permute_intensity_kernel(const float* __restrict__ in, const int* __restrict__ order, int n, float* __restrict__ out)
{
    const int s = blockIdx.x * 256 + (int)threadIdx.x;
    if (s >= n) return;
    out[s] = in[order[s]];
}

}  // namespace

hipError_t color_gradients(const NnGridView& g, const ColorGradientArgs& a, int fma, hipStream_t s)
{
    if (a.q.n < 1 || a.k < 2 || a.k > KNN_MAX_K) return hipErrorInvalidValue;
    knn_dispatch(a.q.n, a.k, fma, [&](auto list, auto fused, dim3 grid) {
        hipLaunchKernelGGL((color_gradient_kernel<decltype(list)::value, decltype(fused)::value>), grid, dim3(KNN_BLOCK), 0, s, g, a);
    });
    return hipGetLastError();
}

hipError_t color_step(const NnGridView& g, const ColorStepArgs& a, int fma, hipStream_t s)
{
    if (a.q.n < 1) return hipErrorInvalidValue;
    const dim3 grid(plane_row_count(a.q.n));
    if (fma) hipLaunchKernelGGL(color_step_kernel<true>, grid, dim3(KNN_BLOCK), 0, s, g, a);
    else hipLaunchKernelGGL(color_step_kernel<false>, grid, dim3(KNN_BLOCK), 0, s, g, a);
    return hipGetLastError();
}

hipError_t color_check_values(const float* v, int count, int* bad, hipStream_t s)
{
    if (count < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(color_check_values_kernel, dim3((count - 1) / 256 + 1), dim3(256), 0, s, v, count, bad);
    return hipGetLastError();
}

hipError_t color_pack_fixed(const float* grad3, const float* intensity, int m, float4* packed, int* bad_intensity, int* bad_gradient, hipStream_t s)
{
    if (m < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(color_pack_fixed_kernel, dim3((m - 1) / 256 + 1), dim3(256), 0, s, grad3, intensity, m, packed, bad_intensity, bad_gradient);
    return hipGetLastError();
}

hipError_t color_permute_intensity(const float* in, const int* order, int n, float* out, hipStream_t s)
{
    if (n < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(color_permute_intensity_kernel, dim3((n - 1) / 256 + 1), dim3(256), 0, s, in, order, n, out);
    return hipGetLastError();
}

// loads this translation unit's code object at mi_ctx_preload (kernels.h)
__global__ void preload_color_kernels_kernel() {}
hipError_t preload_color_kernels()
{
    hipFuncAttributes attr;
    return hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(preload_color_kernels_kernel));
}

}  // namespace mislam
