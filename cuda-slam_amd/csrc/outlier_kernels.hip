// K15 -- statistical and radius outlier removal (mi_remove_outliers; driver: outlier_api.hip).
//
//   score    statistical.  One launch does the search and the score, in the shape of K14: the search is K13's in self mode, the body of
//            knn_scan.hpp, and behind it the lane holds its point's neighbours as K sorted keys in registers -- the keys mi_knn_search would
//            have written out.  They are walked with static indices, predicated on "slot filled": sum += sqrt((double)d2), nearest first, a
//            fixed order; the score is sum / count in fp64 (0 where count is 0), written unrounded to row order[s].  No LDS, no scratch.
//   count    radius.  radius_scan (knn_scan.hpp): the same walk with a counter in the place of the list, stopped by the same bound against r2.
//            EARLY leaves the loops at min_neighbours: the flag is the same, the count is not the whole one.
//   stats    two passes over the n scores, each a grid-stride sum into one partial per workgroup (block_sum_store) and one workgroup
//            over the partials in a fixed order (reduce_partials): the sum -> mean; the squared deviations about it -> stddev, threshold.
//            The number of workgroups is a function of n alone, so the same scores give the same bits.  All three stay on the device.
//   flags    in the caller's order: score <= threshold (read from the state), or count >= min_neighbours.
//   compact  exclusive scan of the flags: ones per tile of 1024, one workgroup scans the tiles' counts (its total is the kept count), then
//            every tile scans its own flags and scatters the indices of its ones, ascending, and their points' bits.  No atomics anywhere.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "knn_scan.hpp"
#include "nn_grid.h"
#include "reduce.hpp"

namespace mislam {

namespace {

template <int K, bool FMA>
__global__ __launch_bounds__(KNN_BLOCK) void knn_outlier_score_kernel(NnGridView g, KnnOutlierArgs a)
{
    float q[3];
    int row_out;
    if (!knn_lane(a.q, q, row_out)) return;
    const int k = a.k;

    unsigned long long l[K];
#pragma unroll
    for (int i = 0; i < K; i++) l[i] = i < K - k ? 0ull : KNN_KEY_EMPTY;
    knn_scan<K, FMA>(g, q, a.q.hi, (unsigned int)row_out, k, __builtin_inff(), l);

    double sum = 0.0;
    int found = 0;
#pragma unroll
    for (int i = 0; i < K; i++) {
        const unsigned int hi = (unsigned int)(l[i] >> 32);
        if (i >= K - k && hi < 0x7f800000u) {                                       // a filled slot of the k-list
            sum += sqrt((double)__uint_as_float(hi));
            found++;
        }
    }
    a.score[row_out] = found > 0 ? sum / (double)found : 0.0;
    if (a.count) a.count[row_out] = found;
}

template <bool FMA, bool EARLY>
__global__ __launch_bounds__(KNN_BLOCK) void radius_count_kernel(NnGridView g, RadiusCountArgs a)
{
    float q[3];
    int row_out;
    if (!knn_lane(a.q, q, row_out)) return;
    a.count[row_out] = radius_scan<FMA, EARLY>(g, q, a.q.hi, (unsigned int)row_out, a.r2, a.min_neighbours);
}

// ---- statistics: DEV false: the sum of the scores; true: the sum of their squared deviations about state->mean
template <bool DEV>
__global__ __launch_bounds__(OUTLIER_STAT_BLOCK) void outlier_sum_kernel(const double* __restrict__ score, int n, const OutlierState* __restrict__ st,
                                                                         double* __restrict__ partials)
{
    const double mean = DEV ? st->mean : 0.0;
    double acc[1] = {0.0};
    const size_t stride = (size_t)gridDim.x * OUTLIER_STAT_BLOCK;
    for (size_t i = (size_t)blockIdx.x * OUTLIER_STAT_BLOCK + threadIdx.x; i < (size_t)n; i += stride) {
        const double d = score[i] - mean;
        acc[0] += DEV ? d * d : d;
    }
    block_sum_store<1>(acc, partials + blockIdx.x);
}

template <bool DEV>
__global__ __launch_bounds__(256) void outlier_stat_finish_kernel(const double* __restrict__ partials, int nblocks, int n, float std_ratio,
                                                                  OutlierState* __restrict__ st)
{
    __shared__ double lds[256];
    double tot[1];
    reduce_partials<1>(partials, nblocks, tot, lds);
    if (threadIdx.x != 0) return;
    if (!DEV) {
        st->mean = tot[0] / (double)n;
    } else {
        const double sd = sqrt(tot[0] / (double)n);
        st->stddev = sd;
        st->threshold = st->mean + (double)std_ratio * sd;
    }
}

__global__ __launch_bounds__(256) void outlier_flags_statistical_kernel(const double* __restrict__ score, int n, const OutlierState* __restrict__ st,
                                                                        unsigned char* __restrict__ keep, float* __restrict__ mean_distance)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)n) return;
    const double mu = score[i];
    keep[i] = mu <= st->threshold ? 1 : 0;
    if (mean_distance) mean_distance[i] = (float)mu;
}

__global__ __launch_bounds__(256) void outlier_flags_radius_kernel(const int* __restrict__ count, int n, int min_neighbours, unsigned char* __restrict__ keep)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)n) return;
    keep[i] = count[i] >= min_neighbours ? 1 : 0;
}

// ---- compaction
// exclusive scan of one int per lane over a 256-lane workgroup; *total: the sum over the workgroup.  lds: 4 ints, free again on return
__device__ __forceinline__ int block_exclusive_scan(int v, int* lds, int* total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int t = __shfl_up(inc, off, 64);
        if (lane >= off) inc += t;
    }
    if (lane == 63) lds[wave] = inc;
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < 4; w++) {
        const int c = lds[w];
        base += w < wave ? c : 0;
        tot += c;
    }
    __syncthreads();
    *total = tot;
    return base + inc - v;
}

// the lane's four consecutive flags of its tile as bits 0 .. 3 (0 beyond n)
__device__ __forceinline__ unsigned int tile_flags(const unsigned char* __restrict__ keep, int n, size_t first)
{
    unsigned int f = 0;
#pragma unroll
    for (int j = 0; j < 4; j++)
        if (first + j < (size_t)n && keep[first + j]) f |= 1u << j;
    return f;
}

__global__ __launch_bounds__(256) void outlier_tile_count_kernel(const unsigned char* __restrict__ keep, int n, int* __restrict__ tile_counts)
{
    __shared__ int lds[4];
    const size_t first = (size_t)blockIdx.x * OUTLIER_SCAN_TILE + 4 * (size_t)threadIdx.x;
    int total;
    (void)block_exclusive_scan(__popc(tile_flags(keep, n, first)), lds, &total);
    if (threadIdx.x == 0) tile_counts[blockIdx.x] = total;
}

// one workgroup: tile_counts[t] <- the ones before tile t; state->kept <- the ones of all tiles.  Lane i takes a run of consecutive tiles.
__global__ __launch_bounds__(256) void outlier_tile_scan_kernel(int* __restrict__ tile_counts, int tiles, OutlierState* __restrict__ st)
{
    __shared__ int lds[4];
    const int per = (tiles + 255) / 256;
    const int lo = min((int)threadIdx.x * per, tiles), hi = min(lo + per, tiles);
    int mine = 0;
    for (int t = lo; t < hi; t++) mine += tile_counts[t];
    int total;
    int run = block_exclusive_scan(mine, lds, &total);
    for (int t = lo; t < hi; t++) {
        const int c = tile_counts[t];
        tile_counts[t] = run;
        run += c;
    }
    if (threadIdx.x == 0) st->kept = (long long)total;
}

__global__ __launch_bounds__(256) void outlier_scatter_kernel(OutlierCompactArgs a)
{
    __shared__ int lds[4];
    const size_t first = (size_t)blockIdx.x * OUTLIER_SCAN_TILE + 4 * (size_t)threadIdx.x;
    const unsigned int f = tile_flags(a.keep, a.n, first);
    int total;
    size_t pos = (size_t)a.tile_counts[blockIdx.x] + (size_t)block_exclusive_scan(__popc(f), lds, &total);
#pragma unroll
    for (int j = 0; j < 4; j++) {
        if (!((f >> j) & 1u)) continue;
        const size_t i = first + j;                                                 // (< n: tile_flags), pos < the ones of all tiles <= n
        if (a.out_index) a.out_index[pos] = (int)i;
        if (a.out_xyz) {
            a.out_xyz[3 * pos] = a.xyz[3 * i]; a.out_xyz[3 * pos + 1] = a.xyz[3 * i + 1]; a.out_xyz[3 * pos + 2] = a.xyz[3 * i + 2];
        }
        pos++;
    }
}

}  // namespace

hipError_t knn_outlier_score(const NnGridView& g, const KnnOutlierArgs& a, int fma, hipStream_t s)
{
    if (a.q.n < 1 || a.k < 1 || a.k > KNN_MAX_K || !a.score) return hipErrorInvalidValue;
    knn_dispatch(a.q.n, a.k, fma, [&](auto list, auto fused, dim3 grid) {
        hipLaunchKernelGGL((knn_outlier_score_kernel<decltype(list)::value, decltype(fused)::value>), grid, dim3(KNN_BLOCK), 0, s, g, a);
    });
    return hipGetLastError();
}

hipError_t radius_count(const NnGridView& g, const RadiusCountArgs& a, int fma, int early, hipStream_t s)
{
    if (a.q.n < 1 || a.min_neighbours < 1 || !(a.r2 >= 0.f) || !a.count) return hipErrorInvalidValue;
    const dim3 grid((a.q.n + KNN_BLOCK - 1) / KNN_BLOCK), block(KNN_BLOCK);
    if (fma && early) hipLaunchKernelGGL((radius_count_kernel<true, true>), grid, block, 0, s, g, a);
    else if (fma) hipLaunchKernelGGL((radius_count_kernel<true, false>), grid, block, 0, s, g, a);
    else if (early) hipLaunchKernelGGL((radius_count_kernel<false, true>), grid, block, 0, s, g, a);
    else hipLaunchKernelGGL((radius_count_kernel<false, false>), grid, block, 0, s, g, a);
    return hipGetLastError();
}

int outlier_stat_blocks(int n)
{
    const long long b = ((long long)n + OUTLIER_STAT_BLOCK - 1) / OUTLIER_STAT_BLOCK;
    return (int)(b < 1 ? 1 : (b > OUTLIER_STAT_BLOCKS ? OUTLIER_STAT_BLOCKS : b));
}

int outlier_scan_tiles(int n) { return (int)(((long long)n + OUTLIER_SCAN_TILE - 1) / OUTLIER_SCAN_TILE); }

hipError_t outlier_statistics(const double* score, int n, float std_ratio, double* partials, OutlierState* state, hipStream_t s)
{
    if (n < 1) return hipErrorInvalidValue;
    const int nb = outlier_stat_blocks(n);
    hipLaunchKernelGGL((outlier_sum_kernel<false>), dim3(nb), dim3(OUTLIER_STAT_BLOCK), 0, s, score, n, state, partials);
    hipLaunchKernelGGL((outlier_stat_finish_kernel<false>), dim3(1), dim3(256), 0, s, partials, nb, n, std_ratio, state);
    hipLaunchKernelGGL((outlier_sum_kernel<true>), dim3(nb), dim3(OUTLIER_STAT_BLOCK), 0, s, score, n, state, partials);
    hipLaunchKernelGGL((outlier_stat_finish_kernel<true>), dim3(1), dim3(256), 0, s, partials, nb, n, std_ratio, state);
    return hipGetLastError();
}

hipError_t outlier_flags_statistical(const double* score, int n, const OutlierState* state, unsigned char* keep, float* mean_distance, hipStream_t s)
{
    if (n < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(outlier_flags_statistical_kernel, dim3((unsigned int)(((long long)n + 255) / 256)), dim3(256), 0, s, score, n, state, keep, mean_distance);
    return hipGetLastError();
}

hipError_t outlier_flags_radius(const int* count, int n, int min_neighbours, unsigned char* keep, hipStream_t s)
{
    if (n < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(outlier_flags_radius_kernel, dim3((unsigned int)(((long long)n + 255) / 256)), dim3(256), 0, s, count, n, min_neighbours, keep);
    return hipGetLastError();
}

hipError_t outlier_compact(const OutlierCompactArgs& a, hipStream_t s)
{
    if (a.n < 1) return hipErrorInvalidValue;
    const int tiles = outlier_scan_tiles(a.n);
    hipLaunchKernelGGL(outlier_tile_count_kernel, dim3(tiles), dim3(256), 0, s, a.keep, a.n, a.tile_counts);
    hipLaunchKernelGGL(outlier_tile_scan_kernel, dim3(1), dim3(256), 0, s, a.tile_counts, tiles, a.state);
    if (a.out_index || a.out_xyz) hipLaunchKernelGGL(outlier_scatter_kernel, dim3(tiles), dim3(256), 0, s, a);
    return hipGetLastError();
}

// loads this translation unit's code object at mi_ctx_preload (kernels.h)
__global__ void preload_outlier_kernels_kernel() {}
hipError_t preload_outlier_kernels()
{
    hipFuncAttributes attr;
    return hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(preload_outlier_kernels_kernel));
}

}  // namespace mislam
