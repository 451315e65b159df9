// K51 - K54 -- every neighbour within a radius, as CSR lists (mi_radius_search; driver: radius_api.hip).
//
//   count    K15's full radius count (radius_count, outlier_kernels.hip) in self mode.  That launch skips candidate order[s] whatever the
//            mode, so a separate query set is counted by a twin of it here that skips nothing: the same radius_scan, the same bits.
//   scan     K51.  Exclusive scan of the n int counts into n + 1 long long offsets, the caller's row order: one 64-bit sum per tile of 1024
//            counts, one workgroup over the tiles' sums in a fixed order (its total is offsets[n]), then every tile scans its own counts.
//            Every sum is 64-bit; no atomics.
//   fill     K52.  One lane per query walks the ball a second time (shell_walk, knn_scan.hpp) with RadiusFillSink: every member's key to
//            keys[offsets[row] + found++].  The row's address is formed once, in 64 bits; no int product of a row and a length exists.
//   sort     K53.  One wave per row, every row in place.  Keys within a row are distinct (the index is part of the key), so a key's rank
//            is the number of smaller keys of its row:
//              up to RADIUS_WAVE_ROW keys  one key per lane; the rank is counted over the wave, one v_readlane pair per key of the row
//                                          -- L cross-lane steps for a row of L keys, no LDS -- and the key is stored at its rank;
//              longer                      a bitonic network in its ascending-only form (the first step of a merge mirrors, i with
//                                          i ^ (k - 1); the others compare i with i + j; the smaller key always goes to the lower
//                                          index), over the row padded IN THOUGHT to a power of two: a partner beyond the row's end is a
//                                          key above all others that no step would ever move, so the step is skipped.  Every step with
//                                          both ends inside an aligned chunk of RADIUS_SORT_CHUNK keys runs on that chunk in the LDS;
//                                          the steps that span chunks (rows beyond one chunk) compare in global memory.  Nothing assumes
//                                          that a row fits the LDS, and a row's length alone selects the path: L <= 64 or L > 64.
//            The same kernel, instantiated for the runs of a cell grid, orders every cell's points by index (radius_order_cells): what an
//            unsorted call needs to give the same bits every time, since the grid's build leaves a cell in the order of its atomics.
//   unpack   K54.  keys -> idx and, where asked for, d2; one entry per lane, 64-bit entry numbers.
// No floating-point atomics, no register arrays, no scratch.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "knn_scan.hpp"
#include "nn_grid.h"

namespace mislam {

namespace {

static_assert(RADIUS_SCAN_TILE == 4 * 256, "the scan's tiles: 256 lanes x 4 consecutive counts");
static_assert(RADIUS_WAVE_ROW == 64, "K53's register path: one key per lane of a wave");
static_assert((RADIUS_SORT_CHUNK & (RADIUS_SORT_CHUNK - 1)) == 0 && RADIUS_SORT_CHUNK >= 2 * RADIUS_WAVE_ROW, "K53's chunk: a power of two, at least the shortest long row's network");

template <bool FMA>
__global__ __launch_bounds__(KNN_BLOCK) void radius_query_count_kernel(NnGridView g, SearchQueries v, float r2, int* __restrict__ count)
{
    float q[3];
    int row_out;
    if (!knn_lane(v, q, row_out)) return;
    count[row_out] = radius_scan<FMA, false>(g, q, v.hi, 0xffffffffu, r2, 1);
}

// ---- K51
// exclusive scan of one 64-bit sum per lane over a 256-lane workgroup; *total: the sum over the workgroup.  lds: 4 words, free again on return
__device__ __forceinline__ long long block_exclusive_scan64(long long v, long long* lds, long long* total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const long long t = __shfl_up(inc, off, 64);
        if (lane >= off) inc += t;
    }
    if (lane == 63) lds[wave] = inc;
    __syncthreads();
    long long base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < 4; w++) {
        const long long c = lds[w];
        base += w < wave ? c : 0;
        tot += c;
    }
    __syncthreads();
    *total = tot;
    return base + inc - v;
}

__global__ __launch_bounds__(256) void radius_tile_sum_kernel(const int* __restrict__ count, int n, long long* __restrict__ tile_sums)
{
    __shared__ long long lds[4];
    const size_t first = (size_t)blockIdx.x * RADIUS_SCAN_TILE + 4 * (size_t)threadIdx.x;
    long long mine = 0;
#pragma unroll
    for (int j = 0; j < 4; j++)
        if (first + j < (size_t)n) mine += (long long)count[first + j];
    long long total;
    (void)block_exclusive_scan64(mine, lds, &total);
    if (threadIdx.x == 0) tile_sums[blockIdx.x] = total;
}

// one workgroup: tile_sums[t] <- the members before tile t; *total_out <- the members of all tiles.  Lane i takes a run of consecutive tiles.
__global__ __launch_bounds__(256) void radius_tile_scan_kernel(long long* __restrict__ tile_sums, int tiles, long long* __restrict__ total_out)
{
    __shared__ long long lds[4];
    const int per = (tiles + 255) / 256;
    const int lo = min((int)threadIdx.x * per, tiles), hi = min(lo + per, tiles);
    long long mine = 0;
    for (int t = lo; t < hi; t++) mine += tile_sums[t];
    long long total;
    long long run = block_exclusive_scan64(mine, lds, &total);
    for (int t = lo; t < hi; t++) {
        const long long c = tile_sums[t];
        tile_sums[t] = run;
        run += c;
    }
    if (threadIdx.x == 0) *total_out = total;
}

__global__ __launch_bounds__(256) void radius_offsets_kernel(const int* __restrict__ count, int n, const long long* __restrict__ tile_sums,
                                                             long long* __restrict__ offsets)
{
    __shared__ long long lds[4];
    const size_t first = (size_t)blockIdx.x * RADIUS_SCAN_TILE + 4 * (size_t)threadIdx.x;
    int c[4];
    long long mine = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        c[j] = first + j < (size_t)n ? count[first + j] : 0;
        mine += (long long)c[j];
    }
    long long total;
    long long run = tile_sums[blockIdx.x] + block_exclusive_scan64(mine, lds, &total);
#pragma unroll
    for (int j = 0; j < 4; j++) {
        if (first + j < (size_t)n) offsets[first + j] = run;
        run += (long long)c[j];
    }
}

// ---- K52
template <bool FMA>
__global__ __launch_bounds__(KNN_BLOCK) void radius_fill_kernel(NnGridView g, RadiusFillArgs a)
{
    float q[3];
    int row_out;
    if (!knn_lane(a.q, q, row_out)) return;
    const long long first = a.offsets[row_out];
    int found = 0;
    RadiusFillSink sink{a.self ? (unsigned int)row_out : 0xffffffffu, a.r2, a.keys + first, (int)(a.offsets[row_out + 1] - first), found};
    shell_walk<FMA>(g, q, a.q.hi, sink);
    if (found != sink.room) *a.mismatch = 1;                                          // (never, by construction: the driver refuses the call if it happens)
}

// ---- K53
// What the sort kernel orders: rows of an array, each with a first element and a length, and the key an element is ranked by.
//   T data[]; span(r, first, len); K key(T); T pad(): an element whose key is above every real one; K bcast(K, lane): lane's key to the wave
struct KeyRows {                     // the rows of mi_radius_search: packed keys between 64-bit offsets
    using T = unsigned long long;
    using K = unsigned long long;
    const long long* offsets;
    T* data;
    long long rows;
    __device__ __forceinline__ void span(long long r, long long& first, unsigned int& len) const
    {
        first = offsets[r];
        len = (unsigned int)(offsets[r + 1] - first);                              // (a row is at most the cloud: below 2^31)
    }
    static __device__ __forceinline__ K key(T v) { return v; }
    static __device__ __forceinline__ T pad() { return ~0ull; }
    static __device__ __forceinline__ K bcast(K k, int lane)
    {
        const unsigned int lo = (unsigned int)__builtin_amdgcn_readlane((int)(unsigned int)k, lane);
        const unsigned int hi = (unsigned int)__builtin_amdgcn_readlane((int)(unsigned int)(k >> 32), lane);
        return ((unsigned long long)hi << 32) | lo;
    }
};
typedef unsigned int CellPoint __attribute__((ext_vector_type(4)));              // a float4's bits as a native vector: x, y, z, index
static_assert(sizeof(CellPoint) == sizeof(float4) && alignof(CellPoint) == alignof(float4), "CellPoint is a float4's bits");
struct CellRuns {                    // the runs of a cell grid: points between the cells' offsets, ranked by index (w)
    using T = CellPoint;
    using K = unsigned int;
    const unsigned int* cell_start;
    T* data;
    long long rows;
    __device__ __forceinline__ void span(long long r, long long& first, unsigned int& len) const
    {
        const unsigned int b = cell_start[r];
        first = (long long)b;
        len = cell_start[r + 1] - b;
    }
    static __device__ __forceinline__ K key(T v) { return v.w; }
    static __device__ __forceinline__ T pad() { return T{0u, 0u, 0u, 0xffffffffu}; }
    static __device__ __forceinline__ K bcast(K k, int lane) { return (unsigned int)__builtin_amdgcn_readlane((int)k, lane); }
};

// slot t of a step at distance j (a power of two) -> the lower index of its pair: t's bits from j upwards move one place up
__device__ __forceinline__ unsigned int sort_lower(unsigned int t, unsigned int j) { return ((t & ~(j - 1u)) << 1) | (t & (j - 1u)); }

template <class R>
__device__ __forceinline__ void sort_exchange(typename R::T* a, typename R::T* b)
{
    const typename R::T va = *a, vb = *b;
    if (R::key(vb) < R::key(va)) { *a = vb; *b = va; }
}

// the steps of one merge at distances j_hi, j_hi / 2 ... 1 over the `width` elements in the LDS (width a power of two, j_hi < width)
template <class R>
__device__ __forceinline__ void sort_lds_steps(typename R::T* lds, unsigned int width, unsigned int j_hi)
{
    for (unsigned int j = j_hi; j >= 1u; j >>= 1) {
        for (unsigned int t = threadIdx.x; t < width / 2u; t += 64u) {
            const unsigned int i = sort_lower(t, j);
            sort_exchange<R>(lds + i, lds + i + j);
        }
        __syncthreads();
    }
}

template <class R>
__global__ __launch_bounds__(64) void radius_sort_kernel(R rows)
{
    using T = typename R::T;
    using K = typename R::K;
    constexpr unsigned int C = RADIUS_SORT_CHUNK;
    __shared__ T lds[C];
    const unsigned int lane = threadIdx.x;
    for (long long r = blockIdx.x; r < rows.rows; r += gridDim.x) {
        long long first;
        unsigned int L;
        rows.span(r, first, L);
        if (L < 2u) continue;
        T* row = rows.data + first;
        if (L <= (unsigned int)RADIUS_WAVE_ROW) {
            // one key per lane; its rank is the number of smaller keys of the row
            const T v = lane < L ? row[lane] : R::pad();
            const K k = R::key(v);
            unsigned int rank = 0;
            for (unsigned int j = 0; j < L; j++) rank += R::bcast(k, (int)j) < k ? 1u : 0u;
            if (lane < L) row[rank] = v;                                          // (every lane's load is behind it: the ranks needed all of them)
            continue;
        }
        // the row padded in thought to P, a power of two: elements [L, P) are pad(), and no step moves one
        const unsigned int P = 1u << (32 - __clz((int)(L - 1u)));
        const unsigned int width = P < C ? P : C;                                  // what a chunk's image in the LDS spans
        // every chunk ascending: all merges up to the chunk's width
        for (unsigned int cb = 0; cb < L; cb += C) {
            for (unsigned int t = lane; t < width; t += 64u) lds[t] = cb + t < L ? row[cb + t] : R::pad();
            __syncthreads();
            for (unsigned int k = 2u; k <= width; k <<= 1) {
                for (unsigned int t = lane; t < width / 2u; t += 64u) {
                    const unsigned int i = sort_lower(t, k >> 1);
                    sort_exchange<R>(lds + i, lds + (i ^ (k - 1u)));
                }
                __syncthreads();
                sort_lds_steps<R>(lds, width, k >> 2);
            }
            for (unsigned int t = lane; t < width; t += 64u)
                if (cb + t < L) row[cb + t] = lds[t];
            __syncthreads();
        }
        // the merges that span chunks: their first steps in global memory, the steps inside a chunk in the LDS again
        for (unsigned int k = 2u * C; k <= P && k != 0u; k <<= 1) {
            for (unsigned int t = lane; t < P / 2u; t += 64u) {
                const unsigned int i = sort_lower(t, k >> 1), p = i ^ (k - 1u);
                if (p < L) sort_exchange<R>(row + i, row + p);
            }
            __syncthreads();
            for (unsigned int j = k >> 2; j >= C; j >>= 1) {
                for (unsigned int t = lane; t < P / 2u; t += 64u) {
                    const unsigned int i = sort_lower(t, j), p = i + j;
                    if (p < L) sort_exchange<R>(row + i, row + p);
                }
                __syncthreads();
            }
            for (unsigned int cb = 0; cb < L; cb += C) {
                for (unsigned int t = lane; t < C; t += 64u) lds[t] = cb + t < L ? row[cb + t] : R::pad();
                __syncthreads();
                sort_lds_steps<R>(lds, C, C >> 1);
                for (unsigned int t = lane; t < C; t += 64u)
                    if (cb + t < L) row[cb + t] = lds[t];
                __syncthreads();
            }
        }
    }
}

// ---- K54
__global__ __launch_bounds__(256) void radius_unpack_kernel(const unsigned long long* __restrict__ keys, long long total, int* __restrict__ idx,
                                                            float* __restrict__ d2)
{
    const long long stride = (long long)gridDim.x * 256;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += stride) {
        const unsigned long long key = keys[e];
        idx[e] = (int)(unsigned int)key;
        if (d2) d2[e] = __uint_as_float((unsigned int)(key >> 32));
    }
}

// one wave per row up to this many workgroups; beyond, a workgroup takes every SORT_GRID_MAX-th row
constexpr long long SORT_GRID_MAX = 1ll << 22;

template <class R>
hipError_t sort_launch(const R& rows, hipStream_t s)
{
    if (rows.rows < 1) return hipErrorInvalidValue;
    const unsigned int grid = (unsigned int)(rows.rows < SORT_GRID_MAX ? rows.rows : SORT_GRID_MAX);
    hipLaunchKernelGGL((radius_sort_kernel<R>), dim3(grid), dim3(64), 0, s, rows);
    return hipGetLastError();
}

}  // namespace

int radius_scan_tiles(int n) { return (int)(((long long)n + RADIUS_SCAN_TILE - 1) / RADIUS_SCAN_TILE); }

hipError_t radius_scan_offsets(const int* count, int n, long long* tile_sums, long long* offsets, hipStream_t s)
{
    if (n < 1 || !count || !tile_sums || !offsets) return hipErrorInvalidValue;
    const int tiles = radius_scan_tiles(n);
    hipLaunchKernelGGL(radius_tile_sum_kernel, dim3(tiles), dim3(256), 0, s, count, n, tile_sums);
    hipLaunchKernelGGL(radius_tile_scan_kernel, dim3(1), dim3(256), 0, s, tile_sums, tiles, offsets + n);
    hipLaunchKernelGGL(radius_offsets_kernel, dim3(tiles), dim3(256), 0, s, count, n, tile_sums, offsets);
    return hipGetLastError();
}

hipError_t radius_query_count(const NnGridView& g, const SearchQueries& q, float r2, int* count, int fma, hipStream_t s)
{
    if (q.n < 1 || !(r2 >= 0.f) || !count) return hipErrorInvalidValue;
    const dim3 grid((q.n + KNN_BLOCK - 1) / KNN_BLOCK), block(KNN_BLOCK);
    if (fma) hipLaunchKernelGGL((radius_query_count_kernel<true>), grid, block, 0, s, g, q, r2, count);
    else hipLaunchKernelGGL((radius_query_count_kernel<false>), grid, block, 0, s, g, q, r2, count);
    return hipGetLastError();
}

hipError_t radius_fill(const NnGridView& g, const RadiusFillArgs& a, int fma, hipStream_t s)
{
    if (a.q.n < 1 || !(a.r2 >= 0.f) || !a.offsets || !a.keys || !a.mismatch) return hipErrorInvalidValue;
    const dim3 grid((a.q.n + KNN_BLOCK - 1) / KNN_BLOCK), block(KNN_BLOCK);
    if (fma) hipLaunchKernelGGL((radius_fill_kernel<true>), grid, block, 0, s, g, a);
    else hipLaunchKernelGGL((radius_fill_kernel<false>), grid, block, 0, s, g, a);
    return hipGetLastError();
}

hipError_t radius_sort_rows(const long long* offsets, long long rows, unsigned long long* keys, hipStream_t s)
{
    if (!offsets || !keys) return hipErrorInvalidValue;
    return sort_launch(KeyRows{offsets, keys, rows}, s);
}

hipError_t radius_order_cells(const unsigned int* cell_start, long long n_cells, float4* pts, hipStream_t s)
{
    if (!cell_start || !pts) return hipErrorInvalidValue;
    return sort_launch(CellRuns{cell_start, reinterpret_cast<CellPoint*>(pts), n_cells}, s);
}

hipError_t radius_unpack(const unsigned long long* keys, long long total, int* idx, float* d2, hipStream_t s)
{
    if (total < 1 || !keys || !idx) return hipErrorInvalidValue;
    const long long blocks = (total + 255) / 256;
    hipLaunchKernelGGL(radius_unpack_kernel, dim3((unsigned int)(blocks < (1ll << 20) ? blocks : (1ll << 20))), dim3(256), 0, s, keys, total, idx, d2);
    return hipGetLastError();
}

// loads this translation unit's code object at mi_ctx_preload (kernels.h)
__global__ void preload_radius_kernels_kernel() {}
hipError_t preload_radius_kernels()
{
    hipFuncAttributes attr;
    return hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(preload_radius_kernels_kernel));
}

}  // namespace mislam
