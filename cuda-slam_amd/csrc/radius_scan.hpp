// K15 -- the fixed-radius sibling of knn_scan (knn_scan.hpp): the same walk over Chebyshev shells of cells around the query's cell, with
// a counter where knn_scan keeps its list.  The stop rule is knn_scan's with the radius in the place of the k-th distance: behind shell r
// every unscanned point's rounded distance is at least `bound` (the proof: the head of knn_kernels.hip; the expressions below are
// knn_scan's, term for term), so the lane stops once bound > r2 -- a point AT r2 counts, hence strictly.  The shell loop ends at the
// grid's largest extent from the cell whatever the bound says.  One lane per query; no LDS, no scratch.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "knn_scan.hpp"
#include "nn_grid.h"
#include "nn_walk.hpp"

namespace mislam {

// The number of grid points j != skip with d2(q, j) <= r2, d2 in the arithmetic of knn_scan.  EARLY: returns as soon as the counter
// reaches `enough` (>= 1), so the answer is min(the number, enough).  hi: the upper corner of the cloud's bounding box.
template <bool FMA, bool EARLY>
__device__ __forceinline__ int radius_scan(const NnGridView& g, const float (&q)[3], const float (&hi)[3], unsigned int skip, float r2, int enough)
{
    const int c[3] = {knn_cell_index(knn_cell_u(q[0], g.ox, g.inv_h), g.nx), knn_cell_index(knn_cell_u(q[1], g.oy, g.inv_h), g.ny),
                      knn_cell_index(knn_cell_u(q[2], g.oz, g.inv_h), g.nz)};
    const float e[3] = {fmaxf(fmaxf(g.ox - q[0], q[0] - hi[0]), 0.f), fmaxf(fmaxf(g.oy - q[1], q[1] - hi[1]), 0.f),
                        fmaxf(fmaxf(g.oz - q[2], q[2] - hi[2]), 0.f)};
    const int r_end = max(max(max(c[0], g.nx - 1 - c[0]), max(c[1], g.ny - 1 - c[1])), max(c[2], g.nz - 1 - c[2]));   // the last shell that holds a cell
    int found = 0;

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
                        if (__float_as_uint(p.w) != skip && d2 <= r2) {
                            found++;
                            if (EARLY && found >= enough) return found;
                        }
                    }
                }
            }
        }
        // everything not yet scanned is at least this far (knn_scan's bound)
        const float lb = fmaxf((float)r - 1e-3f, 0.f) * g.h_lo;
        const float gx = (e[0] + lb) * 0.999999f, gy = (e[1] + lb) * 0.999999f, gz = (e[2] + lb) * 0.999999f;
        const float bound = fminf(fminf(sq3<FMA>(gx, e[1], e[2]), sq3<FMA>(e[0], gy, e[2])), sq3<FMA>(e[0], e[1], gz));
        if (bound > r2) break;
    }
    return found;
}

}  // namespace mislam
