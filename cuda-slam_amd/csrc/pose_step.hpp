// The kernel side of the pose loop, stated once for the step kernels of K16, K17 and K31 (plane_kernels.hip, gicp_kernels.hip,
// ndt_kernels.hip): one lane per sorted slot of the moving cloud, workgroups of one wave (KNN_BLOCK), no LDS.
//   move    the lane rounds the state block's fp64 pose to fp32 and moves its point with it in the stated order,
//           q = ((R0 b_x + R1 b_y) + R2 b_z) + t, every operation rounded (the build has -ffp-contract=off)
//   match   K13's search with a single key (shell_walk with NearestSink, knn_scan.hpp): the key mi_knn_search gives for q with k = 1,
//           bit for bit (K16 and K17; K31 looks its voxels up instead)
//   row     the lane's 21 entries of H, 6 of g and its objective are formed one at a time and summed over the wave (wave_sum,
//           reduce.hpp: a fixed tree), so a lane keeps what the entries are formed from alive and no accumulator; lane 0 writes the row
//           (the layout: pose_block.hpp).  A lane without a pair or term holds zeros in what it passes: its entries are +0.
#pragma once
#include <hip/hip_runtime.h>

#include "knn_scan.hpp"
#include "pose_block.hpp"
#include "reduce.hpp"

namespace mislam {

__device__ __forceinline__ void pose_move(const PlaneState* st, float bx, float by, float bz, float (&q)[3])
{
    q[0] = (((float)st->R[0] * bx + (float)st->R[1] * by) + (float)st->R[2] * bz) + (float)st->t[0];
    q[1] = (((float)st->R[3] * bx + (float)st->R[4] * by) + (float)st->R[5] * bz) + (float)st->t[1];
    q[2] = (((float)st->R[6] * bx + (float)st->R[7] * by) + (float)st->R[8] * bz) + (float)st->t[2];
}

// true: the grid holds a candidate within max_d2 of q at a finite distance, point j (< m: the index the grid build stored) at the
// squared distance of bits d2_bits
template <bool FMA>
__device__ __forceinline__ bool nearest_match(const NnGridView& g, const float (&q)[3], const float (&hi)[3], float max_d2, unsigned int& j,
                                              unsigned int& d2_bits)
{
    NearestSink sink{KNN_KEY_EMPTY, max_d2};
    shell_walk<FMA>(g, q, hi, sink);
    d2_bits = (unsigned int)(sink.best >> 32);
    j = (unsigned int)(sink.best & 0xffffffffull);
    return d2_bits < 0x7f800000u;
}

// H(i, j), i <= j < 6, and g(i): the lane's entries; e, aux, count: its objective and what it adds to the row's two counters (a lane that
// counts adds 1.0: a sum of at most 64 of them is exact)
template <class HEntry, class GEntry>
__device__ __forceinline__ void pose_row_write(int lane, double* __restrict__ row, HEntry&& H, GEntry&& g, double e, double aux, double count)
{
    int k = 0;
#pragma unroll
    for (int i = 0; i < 6; i++) {
#pragma unroll
        for (int j = i; j < 6; j++) {
            const double v = wave_sum(H(i, j));
            if (lane == 0) row[k] = v;
            k++;
        }
    }
#pragma unroll
    for (int i = 0; i < 6; i++) {
        const double v = wave_sum(g(i));
        if (lane == 0) row[PLANE_ROW_G + i] = v;
    }
    const double ee = wave_sum(e), aa = wave_sum(aux), cc = wave_sum(count);
    if (lane == 0) {
        row[PLANE_ROW_E] = ee; row[PLANE_ROW_AUX] = aa; row[PLANE_ROW_COUNT] = cc;
        row[30] = 0.0; row[31] = 0.0;
    }
}

}  // namespace mislam
