// K13 -- EXACT k nearest neighbours through a uniform cell grid over the cloud (mi_knn_search; driver: knn_api.hip).
//
// Contract: row i of the answer = the k smallest keys (bits(d2) << 32) | j over the cloud points j, ascending, d2 in the arithmetic of
// the 1-NN searches (sq3 of nn_walk.hpp on the fp32 differences cloud[j] - query[i]).  The key is a total order, so "the k smallest"
// does not depend on the order in which candidates are met, and the kernel only has to make sure that it skips nothing that belongs.
//
//   check   one pass per array: bounding box of the cloud and the lowest index of a point the call refuses (non-finite, |c| > 1e18),
//           the range pass of cloud_range.hpp under the predicate UsablePoint; read back once, before anything is written
//   index   the cell grid of the 1-NN search, built by grid_build (nn_grid.h) into the call's own buffers: points sorted by cell, w =
//           the caller's index, one offset per cell; a row of cells [x0, x1] is ONE contiguous run of pts
//   search  (its body: knn_scan.hpp, shared with K14's normals_kernels.hip and K15's outlier_kernels.hip)  one lane per query, queries along their curve order so that a
//           wave's lanes visit the same cells.  The running list of
//           K = 8 / 16 / 32 keys lives in REGISTERS, sorted; a candidate is offered only when its key is below the list's last one, and
//           goes in through a fully unrolled chain of K selects (every index static: no scratch).  k < K: the K - k lowest slots hold
//           key 0, which no offer moves (an offer is never below 0), so slots [K - k, K) are the k-list and its last slot the threshold.
//           Candidates come in Chebyshev shells of cells around the query's (clamped) cell c: shell r = the cells with max |i - c| = r
//           inside the grid; per (y, z) row of a shell either the whole x-run (rows on the shell's y / z faces) or its two end cells.
//
// Stop rule.  After shell r every unscanned point p sits in a cell whose index differs from c by >= r + 1 on some axis a.  Cell
// coordinates are u = (p - o) * inv_h, the same fp32 expression at build and for the query, rounding <= 2^-23 * 1024 cells; with
// i_p <= u_p (< i_p + 1 below the last cell) and the query's u in [c, c + 1) -- or beyond the grid on the far side of c when it was
// clamped -- the two differ by more than r cells: |p_a - q_a| >= lb = (r - 1e-3) * h_lo in length (NnGridView::h_lo, the 1-NN scan's
// idiom; 1e-3 cells and h_lo's 1e-5 cover every rounding on the way).  A query outside the box on axis b is at least e_b = max(lo_b -
// q_b, q_b - hi_b) from every point on that axis, and when b = a the two add up (the point lies across the face): |p_a - q_a| >= e_a +
// lb.  Hence, with g = e except g_a = (e_a + lb) shrunk by 1e-6, |fl(p - q)| >= g per axis (rounding is monotone), and the rounded
// distance is >= sq3(g) evaluated like a distance.  The bound is the minimum of that over the three choices of a; the lane stops
// when the bound is STRICTLY above its k-th distance (a point AT the k-th distance with a lower index still belongs in the answer),
// or above the distance limit.  For a query inside the box this is (r h)^2; outside, |q - clamp(q)|^2 + 2 e_a r h + (r h)^2.
// The shell loop ends at the grid's largest extent from c whatever the bound says: no lane can spin.
#include <hip/hip_runtime.h>

#include "cloud_range.hpp"
#include "kernels.h"
#include "knn_scan.hpp"
#include "nn_grid.h"

namespace mislam {

namespace {

__global__ __launch_bounds__(256) void knn_range_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ z,
                                                        int n, float* __restrict__ lo_hi, int* __restrict__ bad)
{
    range_block(SoaPoints{x, y, z}, UsablePoint{}, n, lo_hi, bad);
}

// cloud partials [0, cloud_blocks), query partials [KNN_RANGE_BLOCKS, KNN_RANGE_BLOCKS + query_blocks) -> the state
__global__ __launch_bounds__(256) void knn_range_finish_kernel(const float* __restrict__ lo_hi, const int* __restrict__ bad, int cloud_blocks,
                                                               int query_blocks, KnnState* __restrict__ st)
{
    RangeAcc a;
    if (!range_finish<2>(a, lo_hi, cloud_blocks, bad, bad + KNN_RANGE_BLOCKS, query_blocks)) return;
#pragma unroll
    for (int k = 0; k < 3; k++) { st->lo[k] = a.v[k]; st->hi[k] = a.v[3 + k]; }
    st->bad_cloud = a.bad[0];
    st->bad_query = a.bad[1];
}

template <int K, bool FMA>
__global__ __launch_bounds__(KNN_BLOCK) void knn_search_kernel(NnGridView g, KnnSearchArgs a)
{
    float q[3];
    int row_out;
    if (!knn_lane(SearchQueries{a.qx, a.qy, a.qz, a.order, a.n, {}}, q, row_out)) return;      // (KnnSearchArgs keeps its own fields: kernels.h)
    const unsigned int skip = a.self ? (unsigned int)row_out : 0xffffffffu;      // (no cloud point has index 2^32 - 1)
    const int k = a.k;

    unsigned long long l[K];
#pragma unroll
    for (int i = 0; i < K; i++) l[i] = i < K - k ? 0ull : KNN_KEY_EMPTY;
    knn_scan<K, FMA>(g, q, a.hi, skip, k, a.max_d2, l);      // (knn_scan.hpp: the list and the shell walk, shared with K14)

    int found = 0;
#pragma unroll
    for (int i = 0; i < K; i++) {
        const int slot = i - (K - k);
        if (slot >= 0) {
            const unsigned int hi = (unsigned int)(l[i] >> 32);
            a.idx[(size_t)row_out * (size_t)k + (size_t)slot] = (int)(unsigned int)(l[i] & 0xffffffffull);
            if (a.d2) a.d2[(size_t)row_out * (size_t)k + (size_t)slot] = __uint_as_float(hi);
            found += hi < 0x7f800000u ? 1 : 0;
        }
    }
    if (a.count) a.count[row_out] = found;
}

}  // namespace

hipError_t knn_check_inputs(const float* cx, const float* cy, const float* cz, int m, const float* qx, const float* qy, const float* qz, int n,
                            float* lo_hi, int* bad, KnnState* st, hipStream_t s)
{
    const int cb = range_blocks(m, KNN_RANGE_BLOCKS);
    const int qb = qx ? range_blocks(n, KNN_RANGE_BLOCKS) : 0;
    hipLaunchKernelGGL(knn_range_kernel, dim3(cb), dim3(256), 0, s, cx, cy, cz, m, lo_hi, bad);
    if (qb > 0) hipLaunchKernelGGL(knn_range_kernel, dim3(qb), dim3(256), 0, s, qx, qy, qz, n, lo_hi + 6 * KNN_RANGE_BLOCKS, bad + KNN_RANGE_BLOCKS);
    hipLaunchKernelGGL(knn_range_finish_kernel, dim3(1), dim3(256), 0, s, lo_hi, bad, cb, qb, st);
    return hipGetLastError();
}

int knn_list_size(int k) { return k <= 8 ? 8 : (k <= 16 ? 16 : 32); }

hipError_t knn_search(const NnGridView& g, const KnnSearchArgs& a, int fma, hipStream_t s)
{
    if (a.n < 1 || a.k < 1 || a.k > KNN_MAX_K) return hipErrorInvalidValue;
    knn_dispatch(a.n, a.k, fma, [&](auto list, auto fused, dim3 grid) {
        hipLaunchKernelGGL((knn_search_kernel<decltype(list)::value, decltype(fused)::value>), grid, dim3(KNN_BLOCK), 0, s, g, a);
    });
    return hipGetLastError();
}

// loads this translation unit's code object at mi_ctx_preload (kernels.h)
__global__ void preload_knn_kernels_kernel() {}
hipError_t preload_knn_kernels()
{
    hipFuncAttributes attr;
    return hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(preload_knn_kernels_kernel));
}

}  // namespace mislam
