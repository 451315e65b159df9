// K13 / K14 / K15 / K16 -- the search body of the kernels that walk a cloud's cell grid, stated once: the walk over Chebyshev shells of cells with
// its stop rule (shell_walk; the contract and the proof of the stop rule: the head of knn_kernels.hip), the sorted list of K keys in
// registers that the exact k-NN kernels feed from it (knn_scan), the counter of the fixed-radius kernel (radius_scan) and the single key of
// the plane ICP's match (NearestSink; plane_kernels.hip), the writer of the radius search's lists (RadiusFillSink; radius_kernels.hip), and what the
// kernels share around them: the lane's query (knn_lane) and the host's choice of an instantiation (knn_dispatch).
// knn_search_kernel (knn_kernels.hip) writes the list out; knn_normals_kernel (normals_kernels.hip) and knn_outlier_score_kernel
// (outlier_kernels.hip) go on with the keys still in registers.  One lane per query; no LDS, no scratch: every index into the list is static.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "kernels.h"
#include "nn_grid.h"
#include "nn_walk.hpp"

namespace mislam {

// (the build's expressions, nn_grid.hip: the SAME fp32 operations for the cloud's points and for the queries)
__device__ __forceinline__ float knn_cell_u(float p, float o, float inv_h) { return (p - o) * inv_h; }
__device__ __forceinline__ int knn_cell_index(float u, int n) { return (int)fminf(fmaxf(floorf(u), 0.f), (float)(n - 1)); }

// the sorted list with `key` put in its place and the last entry dropped; the caller has checked key < l[K - 1]
template <int K>
__device__ __forceinline__ void knn_insert(unsigned long long (&l)[K], unsigned long long key)
{
#pragma unroll
    for (int i = K - 1; i >= 1; i--) l[i] = key < l[i - 1] ? l[i - 1] : (key < l[i] ? key : l[i]);
    l[0] = key < l[0] ? key : l[0];
}

// The lane of a search kernel: its sorted slot's query into q and the caller's row that slot answers for (in self mode also the one candidate
// it skips) into row_out; false for a lane beyond the n queries.  (knn_normals_kernel keeps these lines of its own: see there.)
__device__ __forceinline__ bool knn_lane(const SearchQueries& v, float (&q)[3], int& row_out)
{
    const int s = blockIdx.x * KNN_BLOCK + (int)threadIdx.x;
    if (s >= v.n) return false;
    q[0] = v.x[s]; q[1] = v.y[s]; q[2] = v.z[s];
    row_out = v.order[s];
    return true;
}

// Every point of the grid to `sink`, in Chebyshev shells of cells around the cell of query q, until the sink says that no point behind the
// shells walked can matter.  hi: the upper corner of the cloud's bounding box (the lower one is the grid's origin).  The sink, by reference:
//   bool take(float d2, unsigned int j)   candidate j at rounded squared distance d2; true: the lane leaves the walk at once
//   static constexpr bool LEAVES          whether take can say so.  Where it cannot, the walk has no way out of its loops but the shell loop's:
//                                         with the dead exit in the source hipcc lays the row loops out differently and does not unroll the counter's
//   bool stop(float bound) const          behind a shell: every point not yet offered is at least `bound` away (rounded like a distance);
//                                         true once none of them can matter.  STRICTLY above the sink's reach: a point AT the reach belongs.
template <bool FMA, class Sink>
__device__ __forceinline__ void shell_walk(const NnGridView& g, const float (&q)[3], const float (&hi)[3], Sink& sink)
{
    const int c[3] = {knn_cell_index(knn_cell_u(q[0], g.ox, g.inv_h), g.nx), knn_cell_index(knn_cell_u(q[1], g.oy, g.inv_h), g.ny),
                      knn_cell_index(knn_cell_u(q[2], g.oz, g.inv_h), g.nz)};
    // how far outside the cloud's box the query is, per axis, rounded like a distance's difference (box_bound, nn_walk.hpp)
    const float e[3] = {fmaxf(fmaxf(g.ox - q[0], q[0] - hi[0]), 0.f), fmaxf(fmaxf(g.oy - q[1], q[1] - hi[1]), 0.f),
                        fmaxf(fmaxf(g.oz - q[2], q[2] - hi[2]), 0.f)};
    const int r_end = max(max(max(c[0], g.nx - 1 - c[0]), max(c[1], g.ny - 1 - c[1])), max(c[2], g.nz - 1 - c[2]));   // the last shell that holds a cell

    for (int r = 0; r <= r_end; r++) {
        const int z0 = max(c[2] - r, 0), z1 = min(c[2] + r, g.nz - 1), y0 = max(c[1] - r, 0), y1 = min(c[1] + r, g.ny - 1);
        const int xa = c[0] - r, xb = c[0] + r, x0 = max(xa, 0), x1 = min(xb, g.nx - 1);
        for (int iz = z0; iz <= z1; iz++) {
            const bool z_face = iz == c[2] - r || iz == c[2] + r;
            for (int iy = y0; iy <= y1; iy++) {
                const unsigned int row = ((unsigned int)iz * (unsigned int)g.ny + (unsigned int)iy) * (unsigned int)g.nx;
                const bool whole = z_face || iy == c[1] - r || iy == c[1] + r;       // (r = 0: the cell itself)
                // the whole x-run of the row, or its two end cells where they exist
                for (int seg = 0; seg < (whole ? 1 : 2); seg++) {
                    const int sa = whole ? x0 : (seg == 0 ? xa : xb), sb = whole ? x1 : sa;
                    if (sa < 0 || sb > g.nx - 1) continue;
                    const unsigned int b = g.cell_start[row + (unsigned int)sa], end = g.cell_start[row + (unsigned int)sb + 1u];
                    for (unsigned int j = b; j < end; j++) {
                        const float4 p = g.pts[j];
                        const float d2 = sq3<FMA>(p.x - q[0], p.y - q[1], p.z - q[2]);
                        if constexpr (Sink::LEAVES) {
                            if (sink.take(d2, __float_as_uint(p.w))) return;
                        } else {
                            sink.take(d2, __float_as_uint(p.w));
                        }
                    }
                }
            }
        }
        // everything not yet scanned is at least this far (see the head of knn_kernels.hip)
        const float lb = fmaxf((float)r - 1e-3f, 0.f) * g.h_lo;
        const float gx = (e[0] + lb) * 0.999999f, gy = (e[1] + lb) * 0.999999f, gz = (e[2] + lb) * 0.999999f;
        const float bound = fminf(fminf(sq3<FMA>(gx, e[1], e[2]), sq3<FMA>(e[0], gy, e[2])), sq3<FMA>(e[0], e[1], gz));
        if (sink.stop(bound)) break;
    }
}

// the sorted list as a sink: a candidate is offered when its key is below the list's last one; the reach is the k-th distance and the limit
template <int K>
struct KnnListSink {
    static constexpr bool LEAVES = false;
    unsigned long long (&l)[K];
    unsigned int skip;
    float max_d2;
    __device__ __forceinline__ bool take(float d2, unsigned int pj)
    {
        const unsigned long long key = ((unsigned long long)__float_as_uint(d2) << 32) | pj;
        if (key < l[K - 1] && pj != skip && d2 <= max_d2) knn_insert<K>(l, key);
        return false;
    }
    __device__ __forceinline__ bool stop(float bound) const
    {
        const float kth = __uint_as_float((unsigned int)(l[K - 1] >> 32));              // (+inf while the list is not full)
        return bound > kth || bound > max_d2;
    }
};

// The k smallest keys (bits(d2) << 32) | j of query q over the grid's points, ascending in l[K - k, K).  The CALLER initialises the
// list, l[i] = i < K - k ? 0 : KNN_KEY_EMPTY (slots below K - k hold key 0, which no offer moves; unfilled ones stay KNN_KEY_EMPTY): with
// that loop in here hipcc keeps a second copy of the list alive across the shell loop (K = 8: 90 VGPRs instead of 60).
// skip: the one point index that is no candidate (self mode), 0xffffffff for none (no cloud point has index 2^32 - 1).  hi: the upper
// corner of the cloud's bounding box (the lower one is the grid's origin).
template <int K, bool FMA>
__device__ __forceinline__ void knn_scan(const NnGridView& g, const float (&q)[3], const float (&hi)[3], unsigned int skip, int k, float max_d2,
                                         unsigned long long (&l)[K])
{
    KnnListSink<K> sink{l, skip, max_d2};
    shell_walk<FMA>(g, q, hi, sink);
}

// one key as a sink (K16's match): the smallest key (bits(d2) << 32) | j met so far, KNN_KEY_EMPTY until a candidate within max_d2 came; the
// reach is min(best distance, max_d2), with KnnListSink's strict stop -- so the key is row 0 of mi_knn_search with k = 1, bit for bit
struct NearestSink {
    static constexpr bool LEAVES = false;
    unsigned long long best;
    float max_d2;
    __device__ __forceinline__ bool take(float d2, unsigned int pj)
    {
        const unsigned long long key = ((unsigned long long)__float_as_uint(d2) << 32) | pj;
        if (key < best && d2 <= max_d2) best = key;
        return false;
    }
    __device__ __forceinline__ bool stop(float bound) const
    {
        const float nearest = __uint_as_float((unsigned int)(best >> 32));             // (+inf while nothing was taken)
        return bound > nearest || bound > max_d2;
    }
};

// a counter as a sink (K15's radius method): the reach is r2, and a point AT r2 counts
template <bool EARLY>
struct RadiusCountSink {
    static constexpr bool LEAVES = EARLY;
    unsigned int skip;
    float r2;
    int enough;
    int& found;
    __device__ __forceinline__ bool take(float d2, unsigned int pj)
    {
        if (pj != skip && d2 <= r2) {
            found++;
            if (EARLY && found >= enough) return true;
        }
        return false;
    }
    __device__ __forceinline__ bool stop(float bound) const { return bound > r2; }
};

// The number of grid points j != skip with d2(q, j) <= r2, d2 in the arithmetic of knn_scan.  EARLY: returns as soon as the counter
// reaches `enough` (>= 1), so the answer is min(the number, enough).  hi: the upper corner of the cloud's bounding box.
template <bool FMA, bool EARLY>
__device__ __forceinline__ int radius_scan(const NnGridView& g, const float (&q)[3], const float (&hi)[3], unsigned int skip, float r2, int enough)
{
    int found = 0;
    RadiusCountSink<EARLY> sink{skip, r2, enough, found};
    shell_walk<FMA>(g, q, hi, sink);
    return found;
}

// a writer as a sink (K52's lists): RadiusCountSink's membership and stop rule, and every member's key (bits(d2) << 32) | j stored at
// row[found++] in the order the walk offers them.  row: the row's first key, a 64-bit address formed once by the caller.  A second walk
// over the same grid meets what the counting walk met, so found ends at the row's length; `room` is that length, and a key beyond it is
// dropped, not stored -- a wrong count must not become a write outside the lists; the kernel reports found != room to the driver.
struct RadiusFillSink {
    static constexpr bool LEAVES = false;
    unsigned int skip;
    float r2;
    unsigned long long* row;
    int room;
    int& found;
    __device__ __forceinline__ bool take(float d2, unsigned int pj)
    {
        if (pj != skip && d2 <= r2) {
            if (found < room) row[found] = ((unsigned long long)__float_as_uint(d2) << 32) | pj;
            found++;
        }
        return false;
    }
    __device__ __forceinline__ bool stop(float bound) const { return bound > r2; }
};

// Host: launch(K, FMA, grid) with the list size of k (knn_list_size) and the distance arithmetic as integral constants, and the grid of one
// lane per query in workgroups of KNN_BLOCK -- the one place that maps (k, fma) to an instantiation of a kernel template.
template <class Launch>
void knn_dispatch(int n, int k, int fma, Launch&& launch)
{
    const dim3 grid((n + KNN_BLOCK - 1) / KNN_BLOCK);
    auto with_list = [&](auto list) {
        if (fma) launch(list, std::true_type{}, grid);
        else launch(list, std::false_type{}, grid);
    };
    switch (knn_list_size(k)) {
        case 8: with_list(std::integral_constant<int, 8>{}); break;
        case 16: with_list(std::integral_constant<int, 16>{}); break;
        default: with_list(std::integral_constant<int, 32>{}); break;
    }
}

}  // namespace mislam
