// Voxel-grid centroids of a cloud: one output point per occupied voxel, the fp64 mean of the voxel's points (mi_voxel_downsample).
//
//   range   per-axis minimum and maximum of the coordinates and the lowest index of a non-finite point: the range pass of
//           cloud_range.hpp under the predicate FinitePoint.  The voxel of a coordinate, floorf((p - o) / v), is monotone in p, so the
//           voxels of the minimum and the maximum ARE the occupied range -- the same pass serves a given origin and the origin it finds
//           itself (the minimum).
//   keys    voxel coordinate minus the axis minimum, per point: packed cx | cy << 10 | cz << 20 when every extent fits ten bits, else
//           one key array per axis (the driver sorts by x, y, z in turn: radix_sort.hip is stable)
//   rows    head flag of a sorted position = its voxel differs from its predecessor's; exclusive scan of the flags, block scan + carry
//           over blocks: the output row of every sorted position, the first position of every row, the row count
//   sums    segmented fp64 sum, ONE LANE PER SORTED POSITION whatever the runs' lengths: a segmented scan over the wave (shuffles), the
//           waves of a workgroup chained through LDS.  A run inside one tile is finished there.  A run that crosses tiles leaves one partial
//           per tile (`back` of the tile it starts in, `front` of every tile it enters) and the fix-up kernel adds them, one wave per
//           run, lanes striding the tiles: a voxel holding the whole cloud costs n / 256 partials, not n terms in one lane.
// Every sum has a fixed order (a function of the sorted order alone) and there is no floating-point atomic: same input, same bits.
#include <hip/hip_runtime.h>

#include "cloud_range.hpp"
#include "kernels.h"
#include "reduce.hpp"

namespace mislam {

namespace {

__global__ __launch_bounds__(256) void vox_range_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ z,
                                                        int n, float* __restrict__ lo_hi, int* __restrict__ bad)
{
    range_block(SoaPoints{x, y, z}, FinitePoint{}, n, lo_hi, bad);
}

__global__ __launch_bounds__(256) void vox_range_finish_kernel(const float* __restrict__ lo_hi, const int* __restrict__ bad, int nblocks,
                                                               int has_origin, float ox, float oy, float oz, float voxel, VoxState* __restrict__ st)
{
    RangeAcc a;
    if (!range_finish<1>(a, lo_hi, nblocks, bad)) return;
    int range_bad = 0;
    const float given[3] = {ox, oy, oz};
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float o = has_origin ? given[k] : a.v[k];
        st->lo[k] = a.v[k]; st->hi[k] = a.v[3 + k]; st->origin[k] = o;
        int c0 = 0, c1 = 0;
        if (!voxel_axis(a.v[k], o, voxel, &c0)) range_bad |= 1 << k;
        if (!voxel_axis(a.v[3 + k], o, voxel, &c1)) range_bad |= 8 << k;
        st->imin[k] = c0; st->imax[k] = c1;
    }
    st->bad_index = a.bad[0];
    st->range_bad = range_bad;
    st->rows = 0;
}

// (the driver has checked the range: every coordinate minus its axis minimum is in [0, 2^20), on the packed path in [0, 2^10))
template <bool PACKED>
__global__ __launch_bounds__(256) void vox_keys_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ z, int n,
                                                       float voxel, const VoxState* __restrict__ st, unsigned int* __restrict__ keys,
                                                       unsigned int* __restrict__ axis_keys, int* __restrict__ vals)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int c[3] = {0, 0, 0};
    (void)voxel_axis(x[i], st->origin[0], voxel, &c[0]);
    (void)voxel_axis(y[i], st->origin[1], voxel, &c[1]);
    (void)voxel_axis(z[i], st->origin[2], voxel, &c[2]);
    const unsigned int kx = (unsigned int)(c[0] - st->imin[0]), ky = (unsigned int)(c[1] - st->imin[1]), kz = (unsigned int)(c[2] - st->imin[2]);
    if (PACKED) keys[i] = kx | (ky << 10) | (kz << 20);
    else {
        keys[i] = kx;
        axis_keys[i] = kx; axis_keys[(size_t)n + i] = ky; axis_keys[2 * (size_t)n + i] = kz;
    }
    vals[i] = i;
}

__global__ __launch_bounds__(256) void vox_gather_keys_kernel(const unsigned int* __restrict__ axis_keys, const int* __restrict__ idx, int n,
                                                              unsigned int* __restrict__ keys)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j < n) keys[j] = axis_keys[idx[j]];
}

// does sorted position j (0 <= j < n) open a run?
template <bool PACKED>
__device__ __forceinline__ bool vox_head(const unsigned int* __restrict__ sorted_keys, const unsigned int* __restrict__ axis_keys,
                                         const int* __restrict__ sorted_idx, int n, int j)
{
    if (j == 0) return true;
    if (PACKED) return sorted_keys[j] != sorted_keys[j - 1];
    const int a = sorted_idx[j], b = sorted_idx[j - 1];
    return axis_keys[a] != axis_keys[b] || axis_keys[(size_t)n + a] != axis_keys[(size_t)n + b] || axis_keys[2 * (size_t)n + a] != axis_keys[2 * (size_t)n + b];
}

// heads per scan tile
template <bool PACKED>
__global__ __launch_bounds__(256) void vox_count_heads_kernel(const unsigned int* __restrict__ sorted_keys, const unsigned int* __restrict__ axis_keys,
                                                              const int* __restrict__ sorted_idx, int n, int* __restrict__ block_heads)
{
    __shared__ int per_wave[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int count = 0;
#pragma unroll
    for (int k = 0; k < VOX_SCAN_TILE / 256; k++) {
        const int j = blockIdx.x * VOX_SCAN_TILE + k * 256 + (int)threadIdx.x;
        const bool head = j < n && vox_head<PACKED>(sorted_keys, axis_keys, sorted_idx, n, j);
        count += (int)__builtin_popcountll(__builtin_amdgcn_ballot_w64(head));       // (the same in every lane of the wave)
    }
    if (lane == 0) per_wave[wave] = count;
    __syncthreads();
    if (threadIdx.x == 0) block_heads[blockIdx.x] = (per_wave[0] + per_wave[1]) + (per_wave[2] + per_wave[3]);
}

// block_heads[b] <- heads before tile b; st->rows <- all heads; run_start[rows] <- n   (one workgroup; 1024 tiles per step)
__global__ __launch_bounds__(1024) void vox_scan_blocks_kernel(int* __restrict__ block_heads, int nblocks, int n, VoxState* __restrict__ st,
                                                               int* __restrict__ run_start)
{
    __shared__ int s[1024];
    int carry = 0;
    for (int b0 = 0; b0 < nblocks; b0 += 1024) {
        const int b = b0 + (int)threadIdx.x;
        const int v = b < nblocks ? block_heads[b] : 0;
        s[threadIdx.x] = v;
        __syncthreads();
        for (int o = 1; o < 1024; o <<= 1) {
            const int t = (int)threadIdx.x >= o ? s[threadIdx.x - o] : 0;
            __syncthreads();
            s[threadIdx.x] += t;
            __syncthreads();
        }
        if (b < nblocks) block_heads[b] = carry + s[threadIdx.x] - v;
        carry += s[1023];
        __syncthreads();
    }
    if (threadIdx.x == 0) { st->rows = carry; run_start[carry] = n; }
}

// row_of[j] = heads in [0, j] - 1; run_start[row] = j at the heads
template <bool PACKED>
__global__ __launch_bounds__(256) void vox_rows_kernel(const unsigned int* __restrict__ sorted_keys, const unsigned int* __restrict__ axis_keys,
                                                       const int* __restrict__ sorted_idx, int n, const int* __restrict__ block_heads,
                                                       int* __restrict__ row_of, int* __restrict__ run_start)
{
    __shared__ int per_wave[VOX_SCAN_TILE / 256][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    bool head[VOX_SCAN_TILE / 256];
    int before_in_wave[VOX_SCAN_TILE / 256];
#pragma unroll
    for (int k = 0; k < VOX_SCAN_TILE / 256; k++) {
        const int j = blockIdx.x * VOX_SCAN_TILE + k * 256 + (int)threadIdx.x;
        head[k] = j < n && vox_head<PACKED>(sorted_keys, axis_keys, sorted_idx, n, j);
        const unsigned long long mask = __builtin_amdgcn_ballot_w64(head[k]);
        before_in_wave[k] = (int)__builtin_popcountll(mask & ((1ull << lane) - 1ull));
        if (lane == 0) per_wave[k][wave] = (int)__builtin_popcountll(mask);
    }
    __syncthreads();
    int carry = block_heads[blockIdx.x];
#pragma unroll
    for (int k = 0; k < VOX_SCAN_TILE / 256; k++) {
        int before = carry;
#pragma unroll
        for (int w = 0; w < 4; w++) {
            if (w < wave) before += per_wave[k][w];
            carry += per_wave[k][w];
        }
        const int j = blockIdx.x * VOX_SCAN_TILE + k * 256 + (int)threadIdx.x;
        if (j < n) {
            const int row = before + before_in_wave[k] + (head[k] ? 1 : 0) - 1;
            row_of[j] = row;
            if (head[k]) run_start[row] = j;
        }
    }
}

// One lane per sorted position: the sum of its run's points from the run's start (or the tile's, if the run entered the tile) up to itself.
__global__ __launch_bounds__(256) void vox_sums_kernel(VoxArgs a)
{
    __shared__ double wave_tail[4][3];       // lane 63 of every wave: its sum ...
    __shared__ int wave_open[4];             // ... and whether its run was already running when the wave began
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int tile = blockIdx.x, tile_lo = tile * VOX_SUM_TILE, wave_lo = tile_lo + wave * 64;
    const int j = tile_lo + (int)threadIdx.x;
    const bool valid = j < a.n;
    int row = 0, start = j, count = 1;
    bool run_end = false;
    double s[3] = {0.0, 0.0, 0.0};
    if (valid) {
        const int i = a.sorted_idx[j];
        row = a.row_of[j];
        start = a.run_start[row];
        const int next = a.run_start[row + 1];
        count = next - start;
        run_end = j == next - 1;
        const float4 p = a.pts[i];
        s[0] = (double)p.x; s[1] = (double)p.y; s[2] = (double)p.z;
        a.voxel_of_point[i] = row;
        if (j == start) {
            a.out_count[row] = count;
            int c[3] = {0, 0, 0};
            (void)voxel_axis(p.x, a.state->origin[0], a.voxel, &c[0]);
            (void)voxel_axis(p.y, a.state->origin[1], a.voxel, &c[1]);
            (void)voxel_axis(p.z, a.state->origin[2], a.voxel, &c[2]);
#pragma unroll
            for (int k = 0; k < 3; k++) a.out_coord[3 * (size_t)row + k] = c[k];
        }
    }
    // segmented inclusive scan over the wave: behind the steps 1 .. off a lane holds the sum of [max(first, j - 2 off + 1), j]
    const int first = max(start, wave_lo);
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        double t[3];
#pragma unroll
        for (int k = 0; k < 3; k++) t[k] = __shfl_up(s[k], off, 64);
        if (valid && j - off >= first) {
#pragma unroll
            for (int k = 0; k < 3; k++) s[k] += t[k];
        }
    }
    if (lane == 63) {
#pragma unroll
        for (int k = 0; k < 3; k++) wave_tail[wave][k] = s[k];
        wave_open[wave] = valid && start < wave_lo ? 1 : 0;
    }
    __syncthreads();
    if (valid && start < wave_lo) {          // the run came in from the waves before: their tails, nearest first, back to where the run started
        double carry[3] = {0.0, 0.0, 0.0};
        for (int w = wave - 1; w >= 0; w--) {
#pragma unroll
            for (int k = 0; k < 3; k++) carry[k] += wave_tail[w][k];
            if (!wave_open[w]) break;
        }
#pragma unroll
        for (int k = 0; k < 3; k++) s[k] += carry[k];
    }
    // s = sum of [max(start, tile_lo), j]
    const bool entered = start < tile_lo;                                       // the run was running when the tile began
    const bool tile_end = valid && !run_end && threadIdx.x == VOX_SUM_TILE - 1;  // ... and goes on behind the tile (run_end holds at j = n - 1)
    if (valid && run_end && !entered) {
#pragma unroll
        for (int k = 0; k < 3; k++) a.out_xyz[3 * (size_t)row + k] = (float)(s[k] / (double)count);
    }
    if ((valid && run_end && entered) || (tile_end && entered)) {
#pragma unroll
        for (int k = 0; k < 3; k++) a.front[3 * (size_t)tile + k] = s[k];
        a.fix[tile] = run_end ? row : -1;
    }
    if (tile_end && !entered) {
#pragma unroll
        for (int k = 0; k < 3; k++) a.back[3 * (size_t)tile + k] = s[k];
    }
    if (threadIdx.x == 0 && !entered) a.fix[tile] = -1;                        // no run enters this tile
}

// One wave per tile: if a run that entered the tile ends in it, its sum = back of the tile it began in + front of every tile it entered.
__global__ __launch_bounds__(256) void vox_fixup_kernel(VoxArgs a, int tiles)
{
    const int lane = threadIdx.x & 63;
    const int tile = blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (tile >= tiles) return;
    const int row = a.fix[tile];
    if (row < 0) return;
    const int start = a.run_start[row], count = a.run_start[row + 1] - start;
    const int first_tile = start / VOX_SUM_TILE;
    double acc[3] = {0.0, 0.0, 0.0};
    for (int t = first_tile + 1 + lane; t <= tile; t += 64) {
#pragma unroll
        for (int k = 0; k < 3; k++) acc[k] += a.front[3 * (size_t)t + k];
    }
#pragma unroll
    for (int k = 0; k < 3; k++) acc[k] = wave_sum(acc[k]);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 3; k++) a.out_xyz[3 * (size_t)row + k] = (float)((a.back[3 * (size_t)first_tile + k] + acc[k]) / (double)count);
    }
}

}  // namespace

hipError_t vox_range(const VoxArgs& a, const float* origin3, hipStream_t s)
{
    const int nb = range_blocks(a.n, VOX_RANGE_BLOCKS);
    hipLaunchKernelGGL(vox_range_kernel, dim3(nb), dim3(256), 0, s, a.x, a.y, a.z, a.n, a.range_lo_hi, a.range_bad);
    hipLaunchKernelGGL(vox_range_finish_kernel, dim3(1), dim3(256), 0, s, a.range_lo_hi, a.range_bad, nb, origin3 ? 1 : 0,
                       origin3 ? origin3[0] : 0.f, origin3 ? origin3[1] : 0.f, origin3 ? origin3[2] : 0.f, a.voxel, a.state);
    return hipGetLastError();
}

hipError_t vox_keys(const VoxArgs& a, hipStream_t s)
{
    const dim3 grid((a.n + 255) / 256);
    if (a.axis_keys == nullptr) hipLaunchKernelGGL(vox_keys_kernel<true>, grid, dim3(256), 0, s, a.x, a.y, a.z, a.n, a.voxel, a.state, a.keys, nullptr, a.vals);
    else hipLaunchKernelGGL(vox_keys_kernel<false>, grid, dim3(256), 0, s, a.x, a.y, a.z, a.n, a.voxel, a.state, a.keys, a.axis_keys, a.vals);
    return hipGetLastError();
}

hipError_t vox_gather_keys(const unsigned int* axis_keys, const int* idx, int n, unsigned int* keys, hipStream_t s)
{
    hipLaunchKernelGGL(vox_gather_keys_kernel, dim3((n + 255) / 256), dim3(256), 0, s, axis_keys, idx, n, keys);
    return hipGetLastError();
}

hipError_t vox_rows(const VoxArgs& a, hipStream_t s)
{
    const int nb = (a.n + VOX_SCAN_TILE - 1) / VOX_SCAN_TILE;
    if (a.axis_keys == nullptr) {
        hipLaunchKernelGGL(vox_count_heads_kernel<true>, dim3(nb), dim3(256), 0, s, a.sorted_keys, nullptr, a.sorted_idx, a.n, a.block_heads);
        hipLaunchKernelGGL(vox_scan_blocks_kernel, dim3(1), dim3(1024), 0, s, a.block_heads, nb, a.n, a.state, a.run_start);
        hipLaunchKernelGGL(vox_rows_kernel<true>, dim3(nb), dim3(256), 0, s, a.sorted_keys, nullptr, a.sorted_idx, a.n, a.block_heads, a.row_of, a.run_start);
    } else {
        hipLaunchKernelGGL(vox_count_heads_kernel<false>, dim3(nb), dim3(256), 0, s, nullptr, a.axis_keys, a.sorted_idx, a.n, a.block_heads);
        hipLaunchKernelGGL(vox_scan_blocks_kernel, dim3(1), dim3(1024), 0, s, a.block_heads, nb, a.n, a.state, a.run_start);
        hipLaunchKernelGGL(vox_rows_kernel<false>, dim3(nb), dim3(256), 0, s, nullptr, a.axis_keys, a.sorted_idx, a.n, a.block_heads, a.row_of, a.run_start);
    }
    return hipGetLastError();
}

hipError_t vox_sums(const VoxArgs& a, hipStream_t s)
{
    const int tiles = (a.n + VOX_SUM_TILE - 1) / VOX_SUM_TILE;
    hipLaunchKernelGGL(vox_sums_kernel, dim3(tiles), dim3(256), 0, s, a);
    hipLaunchKernelGGL(vox_fixup_kernel, dim3((tiles + 3) / 4), dim3(256), 0, s, a, tiles);
    return hipGetLastError();
}

// loads this translation unit's code object at mi_ctx_preload (kernels.h)
__global__ void preload_voxel_kernels_kernel() {}
hipError_t preload_voxel_kernels()
{
    hipFuncAttributes attr;
    return hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(preload_voxel_kernels_kernel));
}

}  // namespace mislam
