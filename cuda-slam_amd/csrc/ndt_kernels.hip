// K27 - K31 -- the Normal Distributions Transform on the device (mi_ndt_voxels, mi_ndt_register, mi_ndt_system; driver: ndt_api.hip).
//
//   K27 scatter   one lane per SORTED position of the voxel filter's order (voxel_kernels.hip has left row_of, run_start and the fp32 means):
//                 d = p - mu in fp64 (mu: the voxel's fp32 mean, promoted), the six products d_a d_b, and vox_sums_kernel's segmented scan
//                 over them -- shuffles over the wave, the waves chained through LDS, one partial per tile for a run that crosses tiles and a
//                 fix-up kernel that adds those, one wave per run.  The order of every sum is a function of the sorted order alone.
//   K28 finish    one lane per voxel: C = Q / (count - 1), eig3.hpp's fp64 Jacobi, the eigenvalue floor, C' and M = C'^-1.
//   K29 check     one lane per LISTED voxel of a registration: finiteness of its mean and matrix, the coordinates' range and strict order
//                 against the row before, every lowest bad row by an integer atomicMin; the coordinates' range and the bounding box of the
//                 means of the rows with a distribution by integer atomicMin / atomicMax (floats as ordered keys); the repack into float4.
//   K30 table     one lane per listed voxel with a distribution claims its slot in the table of voxel_table.hpp, 2 slots per listed voxel.
//                 Keys are unique (the list is strictly ascending), so a lookup finds the same row whatever order the lanes arrived in.
//   K31 step      the lane's move and row are pose_step.hpp's.  The voxel of q by voxel_axis (mi_voxel_index's arithmetic), then per offset of the neighbourhood a
//                 box test on the voxel index, the key, the probe and -- on a hit -- ndt_term.hpp's term, folded into ten running fp64
//                 numbers: A = sum w M (6), b = sum w Md (3), E = sum e.  With P = q - c0 the row's entries are K17's 21 + 6 from A and
//                 b (gicp_terms.hpp), and everything behind the row is plane_reduce_solve.
//                 Per term: 3 subtractions, 9 + 3 products and 6 + 2 additions for Md and m, one exp, 1 + 9 products and 10 additions for
//                 the fold -- about 45 fp64 operations and one exp, against the ~420 of K17's 27 entries, which are paid once per point.
// No float atomics anywhere: the same input gives the same bits on every call.
#include <hip/hip_runtime.h>

#include "eig3.hpp"
#include "gicp_terms.hpp"
#include "kernels.h"
#include "ndt_term.hpp"
#include "pose_step.hpp"
#include "reduce.hpp"

namespace mislam {

namespace {

// ---- K27: vox_sums_kernel's scan with six products about the voxel's mean in the place of the three coordinates
__global__ __launch_bounds__(256) void ndt_scatter_kernel(NdtScatterArgs a)
{
    __shared__ double wave_tail[4][6];       // lane 63 of every wave: its sums ...
    __shared__ int wave_open[4];             // ... and whether its run was already running when the wave began
    const VoxArgs& v = a.v;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int tile = blockIdx.x, tile_lo = tile * VOX_SUM_TILE, wave_lo = tile_lo + wave * 64;
    const int j = tile_lo + (int)threadIdx.x;
    const bool valid = j < v.n;
    int row = 0, start = j;
    bool run_end = false;
    double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (valid) {
        const int i = v.sorted_idx[j];
        row = v.row_of[j];
        start = v.run_start[row];
        run_end = j == v.run_start[row + 1] - 1;
        const float4 p = v.pts[i];
        const double dx = (double)p.x - (double)v.out_xyz[3 * (size_t)row];
        const double dy = (double)p.y - (double)v.out_xyz[3 * (size_t)row + 1];
        const double dz = (double)p.z - (double)v.out_xyz[3 * (size_t)row + 2];
        s[0] = dx * dx; s[1] = dx * dy; s[2] = dx * dz; s[3] = dy * dy; s[4] = dy * dz; s[5] = dz * dz;
    }
    const int first = max(start, wave_lo);
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        double t[6];
#pragma unroll
        for (int k = 0; k < 6; k++) t[k] = __shfl_up(s[k], off, 64);
        if (valid && j - off >= first) {
#pragma unroll
            for (int k = 0; k < 6; k++) s[k] += t[k];
        }
    }
    if (lane == 63) {
#pragma unroll
        for (int k = 0; k < 6; k++) wave_tail[wave][k] = s[k];
        wave_open[wave] = valid && start < wave_lo ? 1 : 0;
    }
    __syncthreads();
    if (valid && start < wave_lo) {          // the run came in from the waves before: their tails, nearest first, back to where the run started
        double carry[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int w = wave - 1; w >= 0; w--) {
#pragma unroll
            for (int k = 0; k < 6; k++) carry[k] += wave_tail[w][k];
            if (!wave_open[w]) break;
        }
#pragma unroll
        for (int k = 0; k < 6; k++) s[k] += carry[k];
    }
    // s = sums over [max(start, tile_lo), j]
    const bool entered = start < tile_lo;
    const bool tile_end = valid && !run_end && threadIdx.x == VOX_SUM_TILE - 1;
    if (valid && run_end && !entered) {
#pragma unroll
        for (int k = 0; k < 6; k++) a.q6[6 * (size_t)row + k] = s[k];
    }
    if ((valid && run_end && entered) || (tile_end && entered)) {
#pragma unroll
        for (int k = 0; k < 6; k++) a.front[6 * (size_t)tile + k] = s[k];
        a.fix[tile] = run_end ? row : -1;
    }
    if (tile_end && !entered) {
#pragma unroll
        for (int k = 0; k < 6; k++) a.back[6 * (size_t)tile + k] = s[k];
    }
    if (threadIdx.x == 0 && !entered) a.fix[tile] = -1;
}

// One wave per tile: if a run that entered the tile ends in it, its sums = back of the tile it began in + front of every tile it entered.
__global__ __launch_bounds__(256) void ndt_scatter_fixup_kernel(NdtScatterArgs a, int tiles)
{
    const int lane = threadIdx.x & 63;
    const int tile = blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (tile >= tiles) return;
    const int row = a.fix[tile];
    if (row < 0) return;
    const int first_tile = a.v.run_start[row] / VOX_SUM_TILE;
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int t = first_tile + 1 + lane; t <= tile; t += 64) {
#pragma unroll
        for (int k = 0; k < 6; k++) acc[k] += a.front[6 * (size_t)t + k];
    }
#pragma unroll
    for (int k = 0; k < 6; k++) acc[k] = wave_sum(acc[k]);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 6; k++) a.q6[6 * (size_t)row + k] = a.back[6 * (size_t)first_tile + k] + acc[k];
    }
}

// ---- K28
__global__ __launch_bounds__(256) void ndt_voxel_finish_kernel(const double* __restrict__ q6, const int* __restrict__ count, const VoxState* __restrict__ st,
                                                               int min_points, float eig_ratio, float* __restrict__ icov6, float* __restrict__ cov6)
{
    const int row = blockIdx.x * 256 + (int)threadIdx.x;
    if (row >= st->rows) return;
    float M[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, Cp[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const int c = count[row];
    if (c >= min_points) {                   // (min_points >= 3: the division below is by 2 at least)
        const double div = (double)(c - 1);
        double Cm[6], lam[3], V[9];
#pragma unroll
        for (int k = 0; k < 6; k++) Cm[k] = q6[6 * (size_t)row + k] / div;
        eig3_symmetric(Cm, lam, V);
        if (lam[2] > 0.0 && lam[2] <= DBL_MAX) {
            const double floor_ = (double)eig_ratio * lam[2];
            const bool raised = lam[0] < floor_ || lam[1] < floor_;
            const double l0 = lam[0] < floor_ ? floor_ : lam[0], l1 = lam[1] < floor_ ? floor_ : lam[1], l2 = lam[2];
            // entry (r, c) of V diag(x) V^T: ((V_r0 x_0) V_c0 + (V_r1 x_1) V_c1) + (V_r2 x_2) V_c2
#define MISLAM_NDT_VXV(r, cc, x0, x1, x2) (((V[3 * r] * (x0)) * V[3 * cc] + (V[3 * r + 1] * (x1)) * V[3 * cc + 1]) + (V[3 * r + 2] * (x2)) * V[3 * cc + 2])
            const double i0 = 1.0 / l0, i1 = 1.0 / l1, i2 = 1.0 / l2;
            M[0] = (float)MISLAM_NDT_VXV(0, 0, i0, i1, i2); M[1] = (float)MISLAM_NDT_VXV(0, 1, i0, i1, i2); M[2] = (float)MISLAM_NDT_VXV(0, 2, i0, i1, i2);
            M[3] = (float)MISLAM_NDT_VXV(1, 1, i0, i1, i2); M[4] = (float)MISLAM_NDT_VXV(1, 2, i0, i1, i2); M[5] = (float)MISLAM_NDT_VXV(2, 2, i0, i1, i2);
            if (raised) {
                Cp[0] = (float)MISLAM_NDT_VXV(0, 0, l0, l1, l2); Cp[1] = (float)MISLAM_NDT_VXV(0, 1, l0, l1, l2); Cp[2] = (float)MISLAM_NDT_VXV(0, 2, l0, l1, l2);
                Cp[3] = (float)MISLAM_NDT_VXV(1, 1, l0, l1, l2); Cp[4] = (float)MISLAM_NDT_VXV(1, 2, l0, l1, l2); Cp[5] = (float)MISLAM_NDT_VXV(2, 2, l0, l1, l2);
            } else {                         // no eigenvalue was raised: C' is C itself
#pragma unroll
                for (int k = 0; k < 6; k++) Cp[k] = (float)Cm[k];
            }
#undef MISLAM_NDT_VXV
        }
    }
#pragma unroll
    for (int k = 0; k < 6; k++) icov6[6 * (size_t)row + k] = M[k];
    if (cov6) {
#pragma unroll
        for (int k = 0; k < 6; k++) cov6[6 * (size_t)row + k] = Cp[k];
    }
}

// ---- K29
__global__ __launch_bounds__(256) void ndt_check_voxels_kernel(const int* __restrict__ coord, const float* __restrict__ mean, const float* __restrict__ icov6, int nv,
                                                               float4* __restrict__ mean4, float4* __restrict__ icov4, NdtMapState* __restrict__ st)
{
    const int i = blockIdx.x * 256 + (int)threadIdx.x;
    if (i >= nv) return;
    const int c[3] = {coord[3 * (size_t)i], coord[3 * (size_t)i + 1], coord[3 * (size_t)i + 2]};
    const float mu[3] = {mean[3 * (size_t)i], mean[3 * (size_t)i + 1], mean[3 * (size_t)i + 2]};
    const float* __restrict__ mp = icov6 + 6 * (size_t)i;
    const float m[6] = {mp[0], mp[1], mp[2], mp[3], mp[4], mp[5]};
    bool mean_ok = true, icov_ok = true, coord_ok = true, some = false;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        mean_ok &= fabsf(mu[k]) <= KNN_MAX_COORD;                                  // (false for NaN and the infinities)
        coord_ok &= c[k] >= -(1 << 30) && c[k] < (1 << 30);
    }
#pragma unroll
    for (int k = 0; k < 6; k++) {
        icov_ok &= fabsf(m[k]) <= KNN_MAX_COORD;
        some |= m[k] != 0.f;
    }
    mean4[i] = make_float4(mu[0], mu[1], mu[2], 0.f);
    icov4[2 * (size_t)i] = make_float4(m[0], m[1], m[2], 0.f);
    icov4[2 * (size_t)i + 1] = make_float4(m[3], m[4], m[5], 0.f);
    if (!mean_ok) atomicMin(&st->bad_mean, i);                                    // (integer minima: the same answer in any order)
    if (!icov_ok) atomicMin(&st->bad_icov, i);
    if (!coord_ok) atomicMin(&st->bad_coord, i);
    if (i > 0) {                             // strictly ascending by (cz, cy, cx) against the row before
        const int p[3] = {coord[3 * (size_t)i - 3], coord[3 * (size_t)i - 2], coord[3 * (size_t)i - 1]};
        const bool above = c[2] != p[2] ? c[2] > p[2] : (c[1] != p[1] ? c[1] > p[1] : c[0] > p[0]);
        if (!above) atomicMin(&st->bad_order, i);
    }
#pragma unroll
    for (int k = 0; k < 3; k++) {
        atomicMin(&st->cmin[k], c[k]);
        atomicMax(&st->cmax[k], c[k]);
    }
    if (some && mean_ok && icov_ok) {
#pragma unroll
        for (int k = 0; k < 3; k++) {
            atomicMin(&st->lo[k], ndt_float_key(mu[k]));
            atomicMax(&st->hi[k], ndt_float_key(mu[k]));
        }
        atomicAdd(&st->with_distribution, 1);
    }
}

// ---- K30.  (the driver has checked the range: every coordinate minus its axis minimum is in [0, ext) with ext <= 2^20)
__global__ __launch_bounds__(256) void ndt_hash_build_kernel(const int* __restrict__ coord, const float4* __restrict__ icov4, int nv, NdtMapView map,
                                                             unsigned long long* __restrict__ keys, int* __restrict__ vals)
{
    const int i = blockIdx.x * 256 + (int)threadIdx.x;
    if (i >= nv) return;
    const float4 m0 = icov4[2 * (size_t)i], m1 = icov4[2 * (size_t)i + 1];
    if (m0.x == 0.f && m0.y == 0.f && m0.z == 0.f && m1.x == 0.f && m1.y == 0.f && m1.z == 0.f) return;      // no distribution: never found
    const VoxelTableView& t = map.table;
    const long long slot = voxel_claim(keys, t.mask, voxel_key(coord[3 * (size_t)i] - t.cmin[0], coord[3 * (size_t)i + 1] - t.cmin[1], coord[3 * (size_t)i + 2] - t.cmin[2]));
    if (slot >= 0) vals[slot] = i;           // (at most nv of the >= 2 nv slots are ever taken)
}

// ---- K31
template <int NB>
__global__ __launch_bounds__(KNN_BLOCK) void ndt_step_kernel(NdtStepArgs a)
{
    const PlaneState* st = a.state;
    if (st->done != 0) return;
    const int lane = (int)threadIdx.x;
    const int s = blockIdx.x * KNN_BLOCK + lane;
    const bool live = s < a.n;

    // (a lane without a term holds zeros in A, b, E and P: its entries are +0)
    NdtPointSums acc;
    ndt_point_clear(&acc);
    double P[3] = {0.0, 0.0, 0.0};
    if (live) {
        float q[3];
        pose_move(st, a.bx[s], a.by[s], a.bz[s], q);
        int c[3] = {0, 0, 0}, own = -1;
        bool inside = voxel_axis(q[0], a.origin[0], a.voxel, &c[0]);             // (false: mi_voxel_index refuses q, NaN and the infinities included)
        inside = voxel_axis(q[1], a.origin[1], a.voxel, &c[1]) && inside;
        inside = voxel_axis(q[2], a.origin[2], a.voxel, &c[2]) && inside;
        if (inside) {
            const double qd[3] = {(double)q[0], (double)q[1], (double)q[2]};
#pragma unroll 1
            for (int o = 0; o < NB; o++) {
                int dx = 0, dy = 0, dz = 0;
                if (NB == 7 && o > 0) {      // -x, +x, -y, +y, -z, +z behind the voxel itself
                    const int axis = (o - 1) >> 1, step = ((o - 1) & 1) ? 1 : -1;
                    dx = axis == 0 ? step : 0; dy = axis == 1 ? step : 0; dz = axis == 2 ? step : 0;
                }
                if (NB == 27) { dz = o / 9 - 1; dy = (o / 3) % 3 - 1; dx = o % 3 - 1; }      // (dz, dy, dx) ascending
                const int row = voxel_row(a.map.table, c[0] + dx, c[1] + dy, c[2] + dz);      // -1: not listed, or listed without a distribution
                if (dx == 0 && dy == 0 && dz == 0) own = row;
                if (row < 0) continue;
                const float4 mu4 = a.map.mean[row], m0 = a.map.icov[2 * (size_t)row], m1 = a.map.icov[2 * (size_t)row + 1];
                const double mu[3] = {(double)mu4.x, (double)mu4.y, (double)mu4.z};
                const double M[6] = {(double)m0.x, (double)m0.y, (double)m0.z, (double)m1.x, (double)m1.y, (double)m1.z};
                NdtTerm t;
                if (ndt_term(qd, mu, M, a.h, a.k, &t)) ndt_point_add(&acc, M, t);
            }
            if (acc.terms > 0) { P[0] = qd[0] - st->c0[0]; P[1] = qd[1] - st->c0[1]; P[2] = qd[2] - st->c0[2]; }
        }
        if (a.idx) a.idx[a.order[s]] = own;
        if (a.terms) a.terms[a.order[s]] = (unsigned char)acc.terms;
    }

    pose_row_write(
        lane, a.rows + (size_t)blockIdx.x * PLANE_ROW, [&](int i, int j) { return gicp_h(acc.A, P, i, j); },
        [&](int i) { return i < 3 ? cross_at(P, i, acc.b[0], acc.b[1], acc.b[2]) : (i == 3 ? acc.b[0] : (i == 4 ? acc.b[1] : acc.b[2])); }, acc.E,
        acc.terms > 0 ? 1.0 : 0.0, (double)acc.terms);
}

}  // namespace

hipError_t ndt_scatter(const NdtScatterArgs& a, hipStream_t s)
{
    if (a.v.n < 1) return hipErrorInvalidValue;
    const int tiles = (a.v.n + VOX_SUM_TILE - 1) / VOX_SUM_TILE;
    hipLaunchKernelGGL(ndt_scatter_kernel, dim3(tiles), dim3(256), 0, s, a);
    hipLaunchKernelGGL(ndt_scatter_fixup_kernel, dim3((tiles + 3) / 4), dim3(256), 0, s, a, tiles);
    return hipGetLastError();
}

hipError_t ndt_voxel_finish(const double* q6, const int* count, const VoxState* st, int rows_at_most, int min_points, float eig_ratio, float* icov6, float* cov6,
                            hipStream_t s)
{
    if (rows_at_most < 1 || min_points < 3) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ndt_voxel_finish_kernel, dim3((rows_at_most - 1) / 256 + 1), dim3(256), 0, s, q6, count, st, min_points, eig_ratio, icov6, cov6);
    return hipGetLastError();
}

hipError_t ndt_check_voxels(const int* coord, const float* mean, const float* icov6, int nv, float4* mean4, float4* icov4, NdtMapState* st, hipStream_t s)
{
    if (nv < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ndt_check_voxels_kernel, dim3((nv - 1) / 256 + 1), dim3(256), 0, s, coord, mean, icov6, nv, mean4, icov4, st);
    return hipGetLastError();
}

hipError_t ndt_hash_build(const int* coord, const float4* icov4, int nv, const NdtMapView& map, unsigned long long* keys, int* vals, hipStream_t s)
{
    if (nv < 1 || !voxel_table_holds(map.table.mask, (unsigned long long)nv, 2)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ndt_hash_build_kernel, dim3((nv - 1) / 256 + 1), dim3(256), 0, s, coord, icov4, nv, map, keys, vals);
    return hipGetLastError();
}

hipError_t ndt_step(const NdtStepArgs& a, int neighbourhood, hipStream_t s)
{
    if (a.n < 1) return hipErrorInvalidValue;
    const dim3 grid(plane_row_count(a.n));
    if (neighbourhood == 1) hipLaunchKernelGGL(ndt_step_kernel<1>, grid, dim3(KNN_BLOCK), 0, s, a);
    else if (neighbourhood == 7) hipLaunchKernelGGL(ndt_step_kernel<7>, grid, dim3(KNN_BLOCK), 0, s, a);
    else if (neighbourhood == 27) hipLaunchKernelGGL(ndt_step_kernel<27>, grid, dim3(KNN_BLOCK), 0, s, a);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

// loads this translation unit's code object at mi_ctx_preload (kernels.h)
__global__ void preload_ndt_kernels_kernel() {}
hipError_t preload_ndt_kernels()
{
    hipFuncAttributes attr;
    return hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(preload_ndt_kernels_kernel));
}

}  // namespace mislam
