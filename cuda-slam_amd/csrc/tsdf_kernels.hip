// K68-K78: the kernels of mi_tsdf_integrate, mi_tsdf_extract, mi_tsdf_raycast and mi_tsdf_mesh (kernels.h has the plan; tsdf_ray.hpp and
// tsdf_cast.hpp the arithmetic, which host and device share word for word).  Every kernel is one lane per ray, row, voxel or slot, in
// workgroups of TSDF_BLOCK; none uses scratch, only the mesh's K76 and K78 use LDS (the triangle table), none has a floating-point atomic: the
// only atomics are integer minima, maxima and counts (the same answer in any order) and the tables' compare-and-swap on keys (a key met again
// is left where it is).
#include <hip/hip_runtime.h>

#include <climits>

#include "kernels.h"
#include "tsdf_cast.hpp"
#include "tsdf_mesh_table.hpp"
#include "tsdf_ray.hpp"

namespace mislam {

// the scan of ray i: the last s with offsets[s] <= i (empty scans repeat an offset: the last one of them holds the ray)
__device__ __forceinline__ int tsdf_scan_of(const long long* __restrict__ offsets, int n_scans, long long i)
{
    int lo = 0, hi = n_scans;                // offsets[lo] <= i < offsets[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (offsets[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ int wave_min_int(int v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ int wave_max_int(int v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    return v;
}

// ---- K68
template <bool FILL>
__global__ __launch_bounds__(TSDF_BLOCK) void tsdf_samples_kernel(TsdfSampleArgs a)
{
    const int i = blockIdx.x * TSDF_BLOCK + (int)threadIdx.x;
    const bool live = i < a.rays;
    int bad_point = TSDF_NO_INDEX, bad_range = TSDF_NO_INDEX;
    int lo0 = INT_MAX, lo1 = INT_MAX, lo2 = INT_MAX, hi0 = INT_MIN, hi1 = INT_MIN, hi2 = INT_MIN;
    int n = 0;
    if (live) {
        const float px = a.xyz[3 * (size_t)i], py = a.xyz[3 * (size_t)i + 1], pz = a.xyz[3 * (size_t)i + 2];
        if (!(fabsf(px) <= TSDF_MAX_ABS && fabsf(py) <= TSDF_MAX_ABS && fabsf(pz) <= TSDF_MAX_ABS)) bad_point = i;
        else {
            const int scan = tsdf_scan_of(a.offsets, a.n_scans, (long long)i);
            float w[3], o[3];
            tsdf_move(a.poses ? a.poses + 16 * (size_t)scan : nullptr, px, py, pz, w, o);
            TsdfRay r;
            if (tsdf_ray(w, o, a.min_range, a.max_range, &r)) {
                const float origin[3] = {a.origin[0], a.origin[1], a.origin[2]};
                size_t at = 0, room = 0;             // (the fill is the count's own code on the same operands; it still never writes past its share)
                if (FILL) { at = (size_t)a.base + (size_t)a.sample_off[i]; room = (size_t)(a.sample_off[i + 1] - a.sample_off[i]); }
                const bool ok = tsdf_walk(r, a.half_steps, a.voxel, origin, a.truncation, [&](int, const int c[3], double f) {
                    if (FILL && (size_t)n < room) {
                        const unsigned int kx = (unsigned int)(c[0] - a.cmin[0]), ky = (unsigned int)(c[1] - a.cmin[1]), kz = (unsigned int)(c[2] - a.cmin[2]);
                        const size_t e = at + (size_t)n;
                        a.keys[e] = kx;
                        a.axis_keys[e] = kx; a.axis_keys[a.entries + e] = ky; a.axis_keys[2 * a.entries + e] = kz;
                        a.vals[e] = (int)e;
                        a.value[e - (size_t)a.base] = f;
                    } else {
                        lo0 = min(lo0, c[0]); lo1 = min(lo1, c[1]); lo2 = min(lo2, c[2]);
                        hi0 = max(hi0, c[0]); hi1 = max(hi1, c[1]); hi2 = max(hi2, c[2]);
                    }
                    n++;
                });
                if (!ok) bad_range = i;
            }
        }
        if (!FILL) a.count[i] = n;
    }
    if (FILL) return;
    // the facts of the wave, then one set of integer atomics per wave (a refused call's ranges are not read)
    bad_point = wave_min_int(bad_point); bad_range = wave_min_int(bad_range);
    lo0 = wave_min_int(lo0); lo1 = wave_min_int(lo1); lo2 = wave_min_int(lo2);
    hi0 = wave_max_int(hi0); hi1 = wave_max_int(hi1); hi2 = wave_max_int(hi2);
    if ((threadIdx.x & 63) == 0) {
        if (bad_point != TSDF_NO_INDEX) atomicMin(&a.state->bad_point, bad_point);
        if (bad_range != TSDF_NO_INDEX) atomicMin(&a.state->bad_range, bad_range);
        if (lo0 <= hi0) {
            atomicMin(&a.state->cmin[0], lo0); atomicMin(&a.state->cmin[1], lo1); atomicMin(&a.state->cmin[2], lo2);
            atomicMax(&a.state->cmax[0], hi0); atomicMax(&a.state->cmax[1], hi1); atomicMax(&a.state->cmax[2], hi2);
        }
    }
}

hipError_t tsdf_samples(const TsdfSampleArgs& a, bool fill, hipStream_t s)
{
    if (a.rays < 1 || !a.xyz || !a.offsets || !a.state || !a.count || a.half_steps < 0 || a.half_steps > TSDF_MAX_HALF_STEPS) return hipErrorInvalidValue;
    if (fill && (!a.sample_off || !a.keys || !a.axis_keys || !a.vals || !a.value)) return hipErrorInvalidValue;
    const dim3 grid((a.rays - 1) / TSDF_BLOCK + 1), block(TSDF_BLOCK);
    if (fill) hipLaunchKernelGGL(tsdf_samples_kernel<true>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(tsdf_samples_kernel<false>, grid, block, 0, s, a);
    return hipGetLastError();
}

// ---- K69
__global__ __launch_bounds__(TSDF_BLOCK) void tsdf_map_keys_kernel(const int* __restrict__ coord, int nv, int c0, int c1, int c2, size_t entries,
                                                                   unsigned int* __restrict__ keys, unsigned int* __restrict__ axis_keys, int* __restrict__ vals)
{
    const int i = blockIdx.x * TSDF_BLOCK + (int)threadIdx.x;
    if (i >= nv) return;
    const unsigned int kx = (unsigned int)(coord[3 * (size_t)i] - c0), ky = (unsigned int)(coord[3 * (size_t)i + 1] - c1), kz = (unsigned int)(coord[3 * (size_t)i + 2] - c2);
    keys[i] = kx;
    axis_keys[i] = kx; axis_keys[entries + i] = ky; axis_keys[2 * entries + i] = kz;
    vals[i] = i;
}

hipError_t tsdf_map_keys(const int* coord, int nv, const int cmin[3], size_t entries, unsigned int* keys, unsigned int* axis_keys, int* vals, hipStream_t s)
{
    if (nv < 1 || (size_t)nv > entries || !coord || !keys || !axis_keys || !vals) return hipErrorInvalidValue;
    hipLaunchKernelGGL(tsdf_map_keys_kernel, dim3((nv - 1) / TSDF_BLOCK + 1), dim3(TSDF_BLOCK), 0, s, coord, nv, cmin[0], cmin[1], cmin[2], entries, keys, axis_keys, vals);
    return hipGetLastError();
}

// ---- K70.  The sort is stable and the entries were numbered (input row, then the samples by ray and k), so a voxel's run is its input row,
// if it has one, and then its samples in ascending (scan, point, k): the lane sums them as they come.
__global__ __launch_bounds__(TSDF_BLOCK) void tsdf_fuse_kernel(TsdfFuseArgs a)
{
    const int row = blockIdx.x * TSDF_BLOCK + (int)threadIdx.x;
    if (row >= a.rows) return;
    int j = a.run_start[row];
    const int end = a.run_start[row + 1];
    const int e0 = a.sorted_idx[j];
    a.out_coord[3 * (size_t)row] = (int)a.axis_keys[e0] + a.cmin[0];
    a.out_coord[3 * (size_t)row + 1] = (int)a.axis_keys[a.entries + e0] + a.cmin[1];
    a.out_coord[3 * (size_t)row + 2] = (int)a.axis_keys[2 * a.entries + e0] + a.cmin[2];
    const bool stored = e0 < a.base;
    if (stored) j++;
    if (stored && j == end) {                // no sample touched it: its bits
        a.out_tsdf[row] = a.in_tsdf[e0];
        a.out_weight[row] = a.in_weight[e0];
        return;
    }
    const double D = stored ? (double)a.in_tsdf[e0] : 0.0, W = stored ? (double)a.in_weight[e0] : 0.0;
    const double C = (double)(end - j);
    double F = 0.0;
    for (; j < end; j++) F += a.value[a.sorted_idx[j] - a.base];
    const double total = W + C, cap = (double)a.max_weight;
    a.out_tsdf[row] = (float)((W * D + F) / total);
    a.out_weight[row] = (float)(total < cap ? total : cap);
}

hipError_t tsdf_fuse(const TsdfFuseArgs& a, hipStream_t s)
{
    if (a.rows < 1 || !a.sorted_idx || !a.run_start || !a.axis_keys || !a.value || !a.out_coord || !a.out_tsdf || !a.out_weight) return hipErrorInvalidValue;
    if (a.base > 0 && (!a.in_tsdf || !a.in_weight)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(tsdf_fuse_kernel, dim3((a.rows - 1) / TSDF_BLOCK + 1), dim3(TSDF_BLOCK), 0, s, a);
    return hipGetLastError();
}

// ---- K71, K72: the observed voxels in voxel_table.hpp's table, voxel_row the row of one or -1.  (the driver has checked the range: every
// coordinate minus its axis minimum is in [0, ext) with ext <= 2^20)
__global__ __launch_bounds__(TSDF_BLOCK) void tsdf_table_kernel(const int* __restrict__ coord, const float* __restrict__ weight, int nv, float min_weight,
                                                                VoxelTableView t, unsigned long long* __restrict__ keys, int* __restrict__ vals)
{
    const int i = blockIdx.x * TSDF_BLOCK + (int)threadIdx.x;
    if (i >= nv || !(weight[i] >= min_weight)) return;
    const long long slot = voxel_claim(keys, t.mask, voxel_key(coord[3 * (size_t)i] - t.cmin[0], coord[3 * (size_t)i + 1] - t.cmin[1], coord[3 * (size_t)i + 2] - t.cmin[2]));
    if (slot >= 0) vals[slot] = i;           // (at most nv of the >= 2 nv slots are ever taken)
}

hipError_t tsdf_table(const int* coord, const float* weight, int nv, float min_weight, const VoxelTableView& t, unsigned long long* keys, int* vals, hipStream_t s)
{
    if (nv < 1 || !voxel_table_holds(t.mask, (unsigned long long)nv, 2) || !coord || !weight || !keys || !vals) return hipErrorInvalidValue;
    hipLaunchKernelGGL(tsdf_table_kernel, dim3((nv - 1) / TSDF_BLOCK + 1), dim3(TSDF_BLOCK), 0, s, coord, weight, nv, min_weight, t, keys, vals);
    return hipGetLastError();
}

// the gradient at the observed voxel (cx, cy, cz) of value f
__device__ __forceinline__ void tsdf_gradient_at(const TsdfCrossArgs& a, int cx, int cy, int cz, double f, double g[3])
{
#pragma unroll
    for (int ax = 0; ax < 3; ax++) {
        const int dx = ax == 0, dy = ax == 1, dz = ax == 2;
        const int m = voxel_row(a.table, cx - dx, cy - dy, cz - dz), p = voxel_row(a.table, cx + dx, cy + dy, cz + dz);
        g[ax] = tsdf_gradient(m >= 0, m >= 0 ? (double)a.tsdf[m] : 0.0, f, p >= 0, p >= 0 ? (double)a.tsdf[p] : 0.0);
    }
}

template <bool FILL>
__global__ __launch_bounds__(TSDF_BLOCK) void tsdf_crossings_kernel(TsdfCrossArgs a)
{
    const int i = blockIdx.x * TSDF_BLOCK + (int)threadIdx.x;
    if (i >= a.nv) return;
    int n = 0;
    if (a.weight[i] >= a.min_weight) {
        const int cx = a.coord[3 * (size_t)i], cy = a.coord[3 * (size_t)i + 1], cz = a.coord[3 * (size_t)i + 2];
        const double f0 = (double)a.tsdf[i];
        bool have_gi = false;
        double gi[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int ax = 0; ax < 3; ax++) {
            const int dx = ax == 0, dy = ax == 1, dz = ax == 2;
            const int j = voxel_row(a.table, cx + dx, cy + dy, cz + dz);
            if (j < 0) continue;
            const double f1 = (double)a.tsdf[j];
            double r;
            if (!tsdf_crossing(f0, f1, &r)) continue;
            if (a.use && !(a.use[i] >> ax & 1)) continue;                       // (mi_tsdf_mesh: a crossing no triangle uses)
            if (FILL && (long long)n < a.offsets[i + 1] - a.offsets[i]) {       // (the count's own code again; never past the row's share)
                const size_t at = 3 *((size_t)a.offsets[i] + (size_t)n);
                a.out_xyz[at] = ax == 0 ? tsdf_crossing_coord(cx, a.origin[0], a.voxel, r) : (float)tsdf_centre(cx, a.origin[0], a.voxel);
                a.out_xyz[at + 1] = ax == 1 ? tsdf_crossing_coord(cy, a.origin[1], a.voxel, r) : (float)tsdf_centre(cy, a.origin[1], a.voxel);
                a.out_xyz[at + 2] = ax == 2 ? tsdf_crossing_coord(cz, a.origin[2], a.voxel, r) : (float)tsdf_centre(cz, a.origin[2], a.voxel);
                if (a.out_normals) {
                    if (!have_gi) { tsdf_gradient_at(a, cx, cy, cz, f0, gi); have_gi = true; }
                    double gj[3];
                    tsdf_gradient_at(a, cx + dx, cy + dy, cz + dz, f1, gj);
                    float nrm[3];
                    tsdf_normal(gi, gj, r, nrm);
                    a.out_normals[at] = nrm[0]; a.out_normals[at + 1] = nrm[1]; a.out_normals[at + 2] = nrm[2];
                }
            }
            n++;
        }
    }
    if (!FILL) a.count[i] = n;
}

hipError_t tsdf_crossings(const TsdfCrossArgs& a, bool fill, hipStream_t s)
{
    if (a.nv < 1 || !a.coord || !a.tsdf || !a.weight || !a.table.keys || !a.table.vals || !a.count) return hipErrorInvalidValue;
    if (fill && (!a.offsets || !a.out_xyz)) return hipErrorInvalidValue;
    const dim3 grid((a.nv - 1) / TSDF_BLOCK + 1), block(TSDF_BLOCK);
    if (fill) hipLaunchKernelGGL(tsdf_crossings_kernel<true>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(tsdf_crossings_kernel<false>, grid, block, 0, s, a);
    return hipGetLastError();
}

// ---- K73, K74: the coarse table of mi_tsdf_raycast's empty-space skipping.  A block is 8^3 voxels, its coordinate the voxel's >> 3; the
// tables are voxel_table.hpp's without values.  Every key of a lane is in [0, ext) of its table (the driver sizes ext from the map's
// range plus one block on either side), every slot index is masked, and at most half the slots are ever taken.
__global__ __launch_bounds__(TSDF_BLOCK) void tsdf_blocks_kernel(const int* __restrict__ coord, const float* __restrict__ weight, int nv, float min_weight,
                                                                 VoxelTableView t, unsigned long long* __restrict__ keys, int* __restrict__ count)
{
    const int i = blockIdx.x * TSDF_BLOCK + (int)threadIdx.x;
    if (i >= nv || !(weight[i] >= min_weight)) return;
    bool fresh;
    voxel_claim(keys, t.mask, voxel_key((coord[3 * (size_t)i] >> TSDF_SKIP_SHIFT) - t.cmin[0], (coord[3 * (size_t)i + 1] >> TSDF_SKIP_SHIFT) - t.cmin[1],
                                        (coord[3 * (size_t)i + 2] >> TSDF_SKIP_SHIFT) - t.cmin[2]), &fresh);
    if (fresh) atomicAdd(count, 1);
}

hipError_t tsdf_blocks(const int* coord, const float* weight, int nv, float min_weight, const VoxelTableView& t, unsigned long long* keys, int* count, hipStream_t s)
{
    if (nv < 1 || !voxel_table_holds(t.mask, (unsigned long long)nv, 2) || !coord || !weight || !keys || !count) return hipErrorInvalidValue;
    hipLaunchKernelGGL(tsdf_blocks_kernel, dim3((nv - 1) / TSDF_BLOCK + 1), dim3(TSDF_BLOCK), 0, s, coord, weight, nv, min_weight, t, keys, count);
    return hipGetLastError();
}

// one lane per slot of K73's table: a block that holds an observed voxel marks itself and its 26 neighbours (they share the table's frame, and
// the frame has a block to spare on every side)
__global__ __launch_bounds__(TSDF_BLOCK) void tsdf_blocks_dilate_kernel(const unsigned long long* __restrict__ held, unsigned long long slots,
                                                                        unsigned long long* __restrict__ keys, unsigned long long mask)
{
    const unsigned long long i = (unsigned long long)blockIdx.x * TSDF_BLOCK + threadIdx.x;
    if (i >= slots) return;
    const unsigned long long key = held[i];
    if (key == VOXEL_KEY_EMPTY) return;
    const int bx = voxel_key_axis(key, 0), by = voxel_key_axis(key, 1), bz = voxel_key_axis(key, 2);
    for (int dz = -1; dz <= 1; dz++)
        for (int dy = -1; dy <= 1; dy++)
            for (int dx = -1; dx <= 1; dx++) voxel_claim(keys, mask, voxel_key(bx + dx, by + dy, bz + dz));
}

hipError_t tsdf_blocks_dilate(const unsigned long long* held, unsigned long long slots, int blocks, unsigned long long* keys, unsigned long long mask, hipStream_t s)
{
    if (slots < 1 || slots > (1ull << 32) || blocks < 1 || !voxel_table_holds(mask, (unsigned long long)blocks, 54) || !held || !keys) return hipErrorInvalidValue;
    hipLaunchKernelGGL(tsdf_blocks_dilate_kernel, dim3((unsigned int)((slots - 1) / TSDF_BLOCK + 1)), dim3(TSDF_BLOCK), 0, s, held, slots, keys, mask);
    return hipGetLastError();
}

// ---- K75: one lane per ray, tsdf_cast.hpp's march over K71's table, the blocks asked of K74's.  Row i of every output is ray i's; a miss writes zeros.
__global__ __launch_bounds__(TSDF_BLOCK) void tsdf_cast_kernel(TsdfCastArgs a)
{
    const int i = blockIdx.x * TSDF_BLOCK + (int)threadIdx.x;
    bool hit = false;
    if (i < a.n) {
        TsdfCastRay ray;
        TsdfCastHit h;
        h.depth = 0.f;
        h.xyz[0] = h.xyz[1] = h.xyz[2] = h.normal[0] = h.normal[1] = h.normal[2] = 0.f;
        if (tsdf_cast_dir(a.has_pose ? a.pose : nullptr, a.dirs[3 * (size_t)i], a.dirs[3 * (size_t)i + 1], a.dirs[3 * (size_t)i + 2], &ray)) {
            TsdfCastGeom g;
            g.origin[0] = a.origin[0]; g.origin[1] = a.origin[1]; g.origin[2] = a.origin[2];
            g.voxel = a.voxel; g.min_range = a.min_range; g.steps = a.steps;
            hit = tsdf_cast(ray, g, a.tsdf, [&](int cx, int cy, int cz) { return voxel_row(a.table, cx, cy, cz); }, a.skip != 0,
                            [&](int bx, int by, int bz) { return voxel_present(a.blocks, bx, by, bz); }, &h);
        }
        a.out_depth[i] = h.depth;
        if (a.out_xyz) { a.out_xyz[3 * (size_t)i] = h.xyz[0]; a.out_xyz[3 * (size_t)i + 1] = h.xyz[1]; a.out_xyz[3 * (size_t)i + 2] = h.xyz[2]; }
        if (a.out_normals) { a.out_normals[3 * (size_t)i] = h.normal[0]; a.out_normals[3 * (size_t)i + 1] = h.normal[1]; a.out_normals[3 * (size_t)i + 2] = h.normal[2]; }
    }
    const unsigned long long hits = __ballot(hit);       // an integer count: the same in any order
    if ((threadIdx.x & 63) == 0 && hits != 0) atomicAdd(a.hits, __popcll(hits));
}

hipError_t tsdf_cast_rays(const TsdfCastArgs& a, hipStream_t s)
{
    if (a.n < 1 || a.steps < 1 || a.steps > TSDF_RAYCAST_MAX_STEPS || !a.dirs || !a.tsdf || !a.table.keys || !a.table.vals || !a.out_depth || !a.hits) return hipErrorInvalidValue;
    if (a.skip && !a.blocks.keys) return hipErrorInvalidValue;
    hipLaunchKernelGGL(tsdf_cast_kernel, dim3((a.n - 1) / TSDF_BLOCK + 1), dim3(TSDF_BLOCK), 0, s, a);
    return hipGetLastError();
}

// ---- K76-K78: marching cubes over K71's table (kernels.h has the plan, mi_slam.h the rules).  Corner c of the cube at a voxel is the voxel
// + (c & 1, (c >> 1) & 1, (c >> 2) & 1); edge e = 4 axis + 2 hi + lo runs along `axis` from its owner corner, whose offset has lo on the
// lower and hi on the higher of the two other axes.
static_assert(TSDF_BLOCK == TSDF_MESH_CASES, "a workgroup stages one row of the table per lane");
__host__ __device__ constexpr int tsdf_mesh_edge_corner(int e)
{
    return (e >> 2) == 0 ? ((e & 1) << 1 | (e & 2) << 1) : ((e >> 2) == 1 ? ((e & 1) | (e & 2) << 1) : ((e & 1) | (e & 2)));
}
static_assert(tsdf_mesh_edge_corner(1) == 2 && tsdf_mesh_edge_corner(3) == 6 && tsdf_mesh_edge_corner(5) == 1 && tsdf_mesh_edge_corner(6) == 4 &&
              tsdf_mesh_edge_corner(7) == 5 && tsdf_mesh_edge_corner(9) == 1 && tsdf_mesh_edge_corner(10) == 2 && tsdf_mesh_edge_corner(11) == 3,
              "the owner corners of mi_slam.h");

__global__ __launch_bounds__(TSDF_BLOCK) void tsdf_mesh_classify_kernel(TsdfMeshArgs a)
{
    __shared__ unsigned long long table[TSDF_MESH_CASES];
    table[threadIdx.x] = TSDF_MESH_TABLE[threadIdx.x];
    __syncthreads();
    const int i = blockIdx.x * TSDF_BLOCK + (int)threadIdx.x;
    if (i >= a.nv) return;
    unsigned int cube = 0;
    int triangles = 0;
    if (a.weight[i] >= a.min_weight) {
        const int cx = a.coord[3 * (size_t)i], cy = a.coord[3 * (size_t)i + 1], cz = a.coord[3 * (size_t)i + 2];
        double f[8];
        bool all = true;
        f[0] = (double)a.tsdf[i];
#pragma unroll
        for (int c = 1; c < 8; c++) {
            const int r = voxel_row(a.table, cx + (c & 1), cy + ((c >> 1) & 1), cz + ((c >> 2) & 1));
            all = all && r >= 0;
            f[c] = r >= 0 ? (double)a.tsdf[r] : 0.0;
        }
        if (all) {
#pragma unroll
            for (int c = 0; c < 8; c++) cube |= (unsigned int)(f[c] > 0.0) << c;
            bool meshed = true;              // every edge whose ends differ in sign is a crossing of K72
#pragma unroll
            for (int e = 0; e < 12; e++) {
                const int c0 = tsdf_mesh_edge_corner(e), c1 = c0 | 1 << (e >> 2);
                double r;
                if ((f[c0] > 0.0) != (f[c1] > 0.0) && !tsdf_crossing(f[c0], f[c1], &r)) meshed = false;
            }
            if (meshed) triangles = (int)(table[cube] >> 60);
        }
    }
    a.cube_case[i] = (unsigned char)cube;
    a.tri_count[i] = triangles;
}

hipError_t tsdf_mesh_classify(const TsdfMeshArgs& a, hipStream_t s)
{
    if (a.nv < 1 || !a.coord || !a.tsdf || !a.weight || !a.table.keys || !a.table.vals || !a.cube_case || !a.tri_count) return hipErrorInvalidValue;
    hipLaunchKernelGGL(tsdf_mesh_classify_kernel, dim3((a.nv - 1) / TSDF_BLOCK + 1), dim3(TSDF_BLOCK), 0, s, a);
    return hipGetLastError();
}

__global__ __launch_bounds__(TSDF_BLOCK) void tsdf_mesh_edges_kernel(TsdfMeshArgs a)
{
    const int i = blockIdx.x * TSDF_BLOCK + (int)threadIdx.x;
    if (i >= a.nv) return;
    unsigned int mask = 0;
    if (a.weight[i] >= a.min_weight) {
        const int c[3] = {a.coord[3 * (size_t)i], a.coord[3 * (size_t)i + 1], a.coord[3 * (size_t)i + 2]};
        const double f0 = (double)a.tsdf[i];
#pragma unroll
        for (int ax = 0; ax < 3; ax++) {
            const int j = voxel_row(a.table, c[0] + (ax == 0), c[1] + (ax == 1), c[2] + (ax == 2));
            if (j < 0) continue;
            double r;
            if (!tsdf_crossing(f0, (double)a.tsdf[j], &r)) continue;
            // the four cubes round the edge: this voxel's and the three a step back along the other axes
            const int u = ax == 0 ? 1 : 0, v = ax == 2 ? 1 : 2;
            bool used = a.tri_count[i] > 0;
#pragma unroll
            for (int k = 1; k < 4 && !used; k++) {
                int d[3] = {0, 0, 0};
                d[u] = k & 1; d[v] = k >> 1;
                const int row = voxel_row(a.table, c[0] - d[0], c[1] - d[1], c[2] - d[2]);
                used = row >= 0 && a.tri_count[row] > 0;
            }
            mask |= (unsigned int)used << ax;
        }
    }
    a.use[i] = (unsigned char)mask;
    a.vert_count[i] = __popc(mask);
}

hipError_t tsdf_mesh_edges(const TsdfMeshArgs& a, hipStream_t s)
{
    if (a.nv < 1 || !a.coord || !a.tsdf || !a.weight || !a.table.keys || !a.table.vals || !a.tri_count || !a.use || !a.vert_count) return hipErrorInvalidValue;
    hipLaunchKernelGGL(tsdf_mesh_edges_kernel, dim3((a.nv - 1) / TSDF_BLOCK + 1), dim3(TSDF_BLOCK), 0, s, a);
    return hipGetLastError();
}

__global__ __launch_bounds__(TSDF_BLOCK) void tsdf_mesh_triangles_kernel(TsdfMeshArgs a)
{
    __shared__ unsigned long long table[TSDF_MESH_CASES];
    __shared__ int corner_row[8][TSDF_BLOCK];            // [corner][lane]: a lane reads and writes its own column alone
    table[threadIdx.x] = TSDF_MESH_TABLE[threadIdx.x];
    __syncthreads();
    const int i = blockIdx.x * TSDF_BLOCK + (int)threadIdx.x;
    if (i >= a.nv) return;
    const long long first = a.tri_off[i];
    const unsigned long long word = table[a.cube_case[i]];
    long long triangles = a.tri_off[i + 1] - first;      // (the count's own words; never past the row's share or the table's row)
    if (triangles > (long long)(word >> 60)) triangles = (long long)(word >> 60);
    if (triangles < 1) return;
    const int cx = a.coord[3 * (size_t)i], cy = a.coord[3 * (size_t)i + 1], cz = a.coord[3 * (size_t)i + 2];
    corner_row[0][threadIdx.x] = i;
#pragma unroll
    for (int c = 1; c < 8; c++) corner_row[c][threadIdx.x] = voxel_row(a.table, cx + (c & 1), cy + ((c >> 1) & 1), cz + ((c >> 2) & 1));
    for (int t = 0; t < (int)triangles; t++) {
#pragma unroll
        for (int v = 0; v < 3; v++) {
            const int e = (int)(word >> 4 * (3 * t + v)) & 15, axis = e >> 2;
            const int owner = e < 12 ? corner_row[tsdf_mesh_edge_corner(e)][threadIdx.x] : -1;
            // the vertex of the crossing (owner, axis): the owner's first vertex plus the used crossings of its lower axes
            a.out_tri[3 * ((size_t)first + (size_t)t) + v] = owner < 0 ? -1 : (int)(a.vert_off[owner] + (long long)__popc(a.use[owner] & ((1u << axis) - 1u)));
        }
    }
}

hipError_t tsdf_mesh_triangles(const TsdfMeshArgs& a, hipStream_t s)
{
    if (a.nv < 1 || !a.coord || !a.table.keys || !a.table.vals || !a.cube_case || !a.use || !a.vert_off || !a.tri_off || !a.out_tri) return hipErrorInvalidValue;
    hipLaunchKernelGGL(tsdf_mesh_triangles_kernel, dim3((a.nv - 1) / TSDF_BLOCK + 1), dim3(TSDF_BLOCK), 0, s, a);
    return hipGetLastError();
}

// Loads this translation unit's code object (mi_ctx_preload).
__global__ void preload_tsdf_kernels_kernel() {}
hipError_t preload_tsdf_kernels()
{
    hipFuncAttributes attr;
    return hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(preload_tsdf_kernels_kernel));
}

}  // namespace mislam
