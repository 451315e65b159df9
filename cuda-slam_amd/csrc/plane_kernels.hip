// K16 -- point-to-plane ICP on the device (mi_icp_plane_register, mi_plane_system; driver: plane_api.hip).  An iteration is two launches
// (three beyond PLANE_ONE_STAGE_ROWS rows), and nothing in it goes through the host:
//
//   step    the lane's move, match and row are pose_step.hpp's.  A lane without a candidate within the limit, or whose matched normal is
//           exactly (0, 0, 0), has no pair.  The pair's numbers in fp64: r = n . (q - a), J = [(q - c0) x n, n]; the row's entries are
//           the products J_i J_j, J_i r and r^2, so a lane keeps J and r alive (the row's layout: pose_block.hpp).
//   sums    the rows are added in a fixed order that depends on their number alone (reduce_partials, reduce.hpp): up to
//           PLANE_ONE_STAGE_ROWS rows by the solve's own workgroup; beyond, PLANE_PARTS workgroups add a slab of rows each first.
//   solve   lane 0 of one workgroup: the stop on too few pairs, plane_solve6 / plane_rodrigues / plane_compose (plane_solve.hpp), the
//           stop rule, all into the state block.  A degenerate system leaves the pose as it was.
// A launch whose state block says "done" returns at once, so a batch of iterations enqueued behind the stop costs empty launches only.
// No float atomics anywhere: the same input gives the same bits on every call.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "knn_scan.hpp"
#include "nn_grid.h"
#include "plane_solve.hpp"
#include "pose_step.hpp"
#include "reduce.hpp"

namespace mislam {

namespace {

template <bool FMA>
__global__ __launch_bounds__(KNN_BLOCK) void plane_step_kernel(NnGridView g, PlaneStepArgs a)
{
    const PlaneState* __restrict__ st = a.state;
    if (st->done != 0) return;
    const int lane = (int)threadIdx.x;
    const int s = blockIdx.x * KNN_BLOCK + lane;
    const bool live = s < a.q.n;

    bool pair = false;
    int match = -1;
    double J0 = 0.0, J1 = 0.0, J2 = 0.0, J3 = 0.0, J4 = 0.0, J5 = 0.0, r = 0.0, d2d = 0.0;
    if (live) {
        float q[3];
        pose_move(st, a.q.x[s], a.q.y[s], a.q.z[s], q);
        unsigned int j, d2_bits;
        if (nearest_match<FMA>(g, q, a.q.hi, a.max_d2, j, d2_bits)) {
            const float4 nf = a.normals[j];
            if (nf.x != 0.f || nf.y != 0.f || nf.z != 0.f) {
                pair = true;
                match = (int)j;
                const double nx = (double)nf.x, ny = (double)nf.y, nz = (double)nf.z;
                const double qx = (double)q[0], qy = (double)q[1], qz = (double)q[2];
                const double dx = qx - (double)a.c.x[j], dy = qy - (double)a.c.y[j], dz = qz - (double)a.c.z[j];
                const double px = qx - st->c0[0], py = qy - st->c0[1], pz = qz - st->c0[2];
                r = (nx * dx + ny * dy) + nz * dz;
                J0 = py * nz - pz * ny; J1 = pz * nx - px * nz; J2 = px * ny - py * nx;
                J3 = nx; J4 = ny; J5 = nz;
                d2d = (double)__uint_as_float(d2_bits);
            }
        }
        if (a.idx) a.idx[a.q.order[s]] = match;
    }

    const double J[6] = {J0, J1, J2, J3, J4, J5};
    pose_row_write(lane, a.rows + (size_t)blockIdx.x * PLANE_ROW, [&](int i, int j) { return J[i] * J[j]; }, [&](int i) { return J[i] * r; }, r * r,
                   d2d, pair ? 1.0 : 0.0);
}

// slab p of `parts` slabs of the rows -> parts_out[p]: rows [p * per, min((p + 1) * per, nrows)), per = ceil(nrows / parts)
__global__ __launch_bounds__(256) void plane_rows_slab_kernel(const PlaneState* __restrict__ st, const double* __restrict__ rows, int nrows, int per,
                                                              double* __restrict__ parts_out)
{
    __shared__ double lds[256];
    if (st->done != 0) return;
    const int lo = min((int)blockIdx.x * per, nrows), cnt = min(per, nrows - lo);
    double out[PLANE_ROW];
    reduce_partials<PLANE_ROW>(rows + (size_t)lo * PLANE_ROW, cnt, out, lds);
#pragma unroll
    for (int i = 0; i < PLANE_ROW; i++)
        if ((int)threadIdx.x == i) parts_out[(size_t)blockIdx.x * PLANE_ROW + i] = out[i];
}

__global__ __launch_bounds__(256) void plane_reduce_solve_kernel(PlaneState* __restrict__ st, const double* __restrict__ rows, int nrows, PlaneRules rules)
{
    __shared__ double lds[256];
    if (st->done != 0) return;
    double sums[PLANE_ROW];
    reduce_partials<PLANE_ROW>(rows, nrows, sums, lds);
    if (threadIdx.x != 0) return;
#pragma unroll
    for (int i = 0; i < PLANE_ROW; i++) st->sums[i] = sums[i];
    if (!rules.solve) return;

    if (sums[PLANE_ROW_COUNT] < (double)PLANE_MIN_PAIRS) { st->done = 1; st->stop_reason = MI_STOP_NO_PAIRS_; return; }
    double A[21], gvec[6], x[6], min_pivot;
#pragma unroll
    for (int i = 0; i < PLANE_ROW_G; i++) A[i] = sums[i];
#pragma unroll
    for (int i = 0; i < 6; i++) gvec[i] = sums[PLANE_ROW_G + i];
    const bool solved = plane_solve6(A, gvec, x, &min_pivot);
    st->min_pivot = min_pivot;
    if (!solved) { st->done = 1; st->stop_reason = MI_STOP_DEGENERATE_; return; }

    const double w[3] = {x[0], x[1], x[2]}, v[3] = {x[3], x[4], x[5]};
    double dR[9], R[9], t[3];
    const double c0[3] = {st->c0[0], st->c0[1], st->c0[2]};
#pragma unroll
    for (int i = 0; i < 9; i++) R[i] = st->R[i];
#pragma unroll
    for (int i = 0; i < 3; i++) t[i] = st->t[i];
    plane_rodrigues(w, dR);
    plane_compose(dR, v, c0, R, t);
#pragma unroll
    for (int i = 0; i < 9; i++) st->R[i] = R[i];
#pragma unroll
    for (int i = 0; i < 3; i++) st->t[i] = t[i];
    const double wn = plane_norm3(w[0], w[1], w[2]), vn = plane_norm3(v[0], v[1], v[2]);
    st->omega = wn; st->v = vn;
    const int it = st->iterations + 1;
    st->iterations = it;
    if (wn <= rules.eps_rotation && vn <= rules.eps_translation) { st->done = 1; st->stop_reason = MI_STOP_CONVERGED_; }
    else if (it >= rules.max_iterations) { st->done = 1; st->stop_reason = MI_STOP_MAX_ITERATIONS_; }
}

}  // namespace

int plane_row_count(int n) { return (n + KNN_BLOCK - 1) / KNN_BLOCK; }
int plane_part_count(int nrows) { return nrows > PLANE_ONE_STAGE_ROWS ? PLANE_PARTS : 0; }

hipError_t plane_step(const NnGridView& g, const PlaneStepArgs& a, int fma, hipStream_t s)
{
    if (a.q.n < 1) return hipErrorInvalidValue;
    const dim3 grid(plane_row_count(a.q.n));
    if (fma) hipLaunchKernelGGL(plane_step_kernel<true>, grid, dim3(KNN_BLOCK), 0, s, g, a);
    else hipLaunchKernelGGL(plane_step_kernel<false>, grid, dim3(KNN_BLOCK), 0, s, g, a);
    return hipGetLastError();
}

hipError_t plane_reduce_solve(PlaneState* state, const double* rows, int nrows, double* parts, const PlaneRules& rules, hipStream_t s)
{
    if (nrows < 1) return hipErrorInvalidValue;
    const int np = plane_part_count(nrows);
    if (np > 0) {
        if (!parts) return hipErrorInvalidValue;
        const int per = (nrows + np - 1) / np;
        hipLaunchKernelGGL(plane_rows_slab_kernel, dim3(np), dim3(256), 0, s, state, rows, nrows, per, parts);
        hipLaunchKernelGGL(plane_reduce_solve_kernel, dim3(1), dim3(256), 0, s, state, parts, np, rules);
    } else {
        hipLaunchKernelGGL(plane_reduce_solve_kernel, dim3(1), dim3(256), 0, s, state, rows, nrows, rules);
    }
    return hipGetLastError();
}

// loads this translation unit's code object at mi_ctx_preload (kernels.h)
__global__ void preload_plane_kernels_kernel() {}
hipError_t preload_plane_kernels()
{
    hipFuncAttributes attr;
    return hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(preload_plane_kernels_kernel));
}

}  // namespace mislam
