// K16 -- point-to-plane ICP on the device (mi_icp_plane_register, mi_plane_system; driver: plane_api.hip).  An iteration is two launches
// (three beyond PLANE_ONE_STAGE_ROWS rows), and nothing in it goes through the host:
//
//   step    one lane per sorted slot of the moving cloud, workgroups of one wave (KNN_BLOCK), no LDS.  The lane rounds the state block's
//           fp64 pose to fp32 and moves its point with it in the stated order, q = ((R0 b_x + R1 b_y) + R2 b_z) + t, every operation
//           rounded (the build has -ffp-contract=off).  Its match is K13's search with a single key (shell_walk with NearestSink,
//           knn_scan.hpp): the key mi_knn_search gives for q with k = 1, bit for bit.  A lane without a candidate within the limit, or
//           whose matched normal is exactly (0, 0, 0), has no pair.  The pair's numbers in fp64: r = n . (q - a), J = [(q - c0) x n, n].
//           The 21 products J_i J_j, the 6 products J_i r, r^2 and d2 are formed one at a time and summed over the wave (wave_sum,
//           reduce.hpp: a fixed tree), so a lane keeps J and r alive and no accumulator; lane 0 writes the row, 32 doubles per 64 slots:
//           [0, 21) sum J J^T, [21, 27) sum J r, [27] sum r^2, [28] sum d2, [29] pairs, [30, 32) 0.
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
    const bool live = s < a.n;

    bool pair = false;
    int match = -1;
    double J0 = 0.0, J1 = 0.0, J2 = 0.0, J3 = 0.0, J4 = 0.0, J5 = 0.0, r = 0.0, d2d = 0.0;
    if (live) {
        const float bx = a.bx[s], by = a.by[s], bz = a.bz[s];
        const float q[3] = {(((float)st->R[0] * bx + (float)st->R[1] * by) + (float)st->R[2] * bz) + (float)st->t[0],
                            (((float)st->R[3] * bx + (float)st->R[4] * by) + (float)st->R[5] * bz) + (float)st->t[1],
                            (((float)st->R[6] * bx + (float)st->R[7] * by) + (float)st->R[8] * bz) + (float)st->t[2]};
        NearestSink sink{KNN_KEY_EMPTY, a.max_d2};
        shell_walk<FMA>(g, q, a.hi, sink);
        const unsigned int d2_bits = (unsigned int)(sink.best >> 32);
        if (d2_bits < 0x7f800000u) {                                                 // a candidate within the limit, at a finite distance
            const unsigned int j = (unsigned int)(sink.best & 0xffffffffull);       // (< m: the index the grid build stored)
            const float4 nf = a.normals[j];
            if (nf.x != 0.f || nf.y != 0.f || nf.z != 0.f) {
                pair = true;
                match = (int)j;
                const double nx = (double)nf.x, ny = (double)nf.y, nz = (double)nf.z;
                const double qx = (double)q[0], qy = (double)q[1], qz = (double)q[2];
                const double dx = qx - (double)a.ax[j], dy = qy - (double)a.ay[j], dz = qz - (double)a.az[j];
                const double px = qx - st->c0[0], py = qy - st->c0[1], pz = qz - st->c0[2];
                r = (nx * dx + ny * dy) + nz * dz;
                J0 = py * nz - pz * ny; J1 = pz * nx - px * nz; J2 = px * ny - py * nx;
                J3 = nx; J4 = ny; J5 = nz;
                d2d = (double)__uint_as_float(d2_bits);
            }
        }
        if (a.idx) a.idx[a.order[s]] = match;
    }

    // (a lane without a pair holds zeros in J, r and d2d: its terms are +0)
    double* __restrict__ row = a.rows + (size_t)blockIdx.x * PLANE_ROW;
    const double J[6] = {J0, J1, J2, J3, J4, J5};
    int k = 0;
#pragma unroll
    for (int i = 0; i < 6; i++) {
#pragma unroll
        for (int j = i; j < 6; j++) {
            const double v = wave_sum(J[i] * J[j]);
            if (lane == 0) row[k] = v;
            k++;
        }
    }
#pragma unroll
    for (int i = 0; i < 6; i++) {
        const double v = wave_sum(J[i] * r);
        if (lane == 0) row[21 + i] = v;
    }
    const double rr = wave_sum(r * r), dd = wave_sum(d2d);
    const int pairs = __popcll(__ballot(pair));
    if (lane == 0) {
        row[27] = rr; row[28] = dd; row[29] = (double)pairs;
        row[30] = 0.0; row[31] = 0.0;
    }
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

    if (sums[29] < (double)PLANE_MIN_PAIRS) { st->done = 1; st->stop_reason = MI_STOP_NO_PAIRS_; return; }
    double A[21], gvec[6], x[6], min_pivot;
#pragma unroll
    for (int i = 0; i < 21; i++) A[i] = sums[i];
#pragma unroll
    for (int i = 0; i < 6; i++) gvec[i] = sums[21 + i];
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
    if (a.n < 1) return hipErrorInvalidValue;
    const dim3 grid(plane_row_count(a.n));
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
