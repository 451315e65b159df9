// K13 / K14 -- the search body of the exact k-NN kernels, stated once: the sorted list of K keys in registers and the walk over
// Chebyshev shells of cells with its stop rule (the contract and the proof of the stop rule: the head of knn_kernels.hip).
// knn_search_kernel (knn_kernels.hip) writes the list out; knn_normals_kernel (normals_kernels.hip) goes on to the neighbourhood's
// covariance with the keys still in registers.  One lane per query; no LDS, no scratch: every index into the list is static.
#pragma once
#include <hip/hip_runtime.h>

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

// The k smallest keys (bits(d2) << 32) | j of query q over the grid's points, ascending in l[K - k, K).  The CALLER initialises the
// list, l[i] = i < K - k ? 0 : KNN_KEY_EMPTY (slots below K - k hold key 0, which no offer moves; unfilled ones stay KNN_KEY_EMPTY): with
// that loop in here hipcc keeps a second copy of the list alive across the shell loop (K = 8: 90 VGPRs instead of 60).
// skip: the one point index that is no candidate (self mode), 0xffffffff for none (no cloud point has index 2^32 - 1).  hi: the upper
// corner of the cloud's bounding box (the lower one is the grid's origin).
template <int K, bool FMA>
__device__ __forceinline__ void knn_scan(const NnGridView& g, const float (&q)[3], const float (&hi)[3], unsigned int skip, int k, float max_d2,
                                         unsigned long long (&l)[K])
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
                        const unsigned int pj = __float_as_uint(p.w);
                        const unsigned long long key = ((unsigned long long)__float_as_uint(d2) << 32) | pj;
                        if (key < l[K - 1] && pj != skip && d2 <= max_d2) knn_insert<K>(l, key);
                    }
                }
            }
        }
        // everything not yet scanned is at least this far (see the head of knn_kernels.hip)
        const float lb = fmaxf((float)r - 1e-3f, 0.f) * g.h_lo;
        const float gx = (e[0] + lb) * 0.999999f, gy = (e[1] + lb) * 0.999999f, gz = (e[2] + lb) * 0.999999f;
        const float bound = fminf(fminf(sq3<FMA>(gx, e[1], e[2]), sq3<FMA>(e[0], gy, e[2])), sq3<FMA>(e[0], e[1], gz));
        const float kth = __uint_as_float((unsigned int)(l[K - 1] >> 32));              // (+inf while the list is not full)
        if (bound > kth || bound > max_d2) break;
    }
}

}  // namespace mislam
