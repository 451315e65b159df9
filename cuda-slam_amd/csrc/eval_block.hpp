// The host arithmetic of mi_evaluate_registration behind the sums (K55, eval_kernels.hip; driver: eval_api.hip): the fitness, the inlier
// RMSE and the 6 x 6 information matrix of a system in pose_block.hpp's layout.  Nothing of HIP is included, so that
// tests/eval_block_selftest.cpp can hold it to its contract on the host alone.
#pragma once
#include <cmath>

#include "pose_block.hpp"

namespace mislam {

// pairs / n, one fp64 division (n >= 1: the entry point refuses an empty moving cloud)
inline double eval_fitness(const double sums[PLANE_ROW], int n) { return sums[PLANE_ROW_COUNT] / (double)n; }

// sqrt(sum |d|^2 / pairs), one fp64 division and one root; 0 with no pair
inline double eval_inlier_rmse(const double sums[PLANE_ROW])
{
    const double pairs = sums[PLANE_ROW_COUNT];
    return pairs > 0.0 ? std::sqrt(sums[PLANE_ROW_E] / pairs) : 0.0;
}

// the slot of entry (i, j) of the 6 x 6 matrix in the row's upper triangle [0, 21), either order of i and j
inline int eval_triangle_slot(int i, int j)
{
    const int r = i < j ? i : j, c = i < j ? j : i;
    return r * 6 - r * (r - 1) / 2 + (c - r);
}

// out (row-major, symmetric) = the expansion of sums[0, 21), the same bits; all +0 with no pair
inline void eval_information(const double sums[PLANE_ROW], double out[36])
{
    const bool any = sums[PLANE_ROW_COUNT] > 0.0;
    for (int i = 0; i < 6; i++)
        for (int j = 0; j < 6; j++) out[6 * i + j] = any ? sums[eval_triangle_slot(i, j)] : 0.0;
}

}  // namespace mislam
