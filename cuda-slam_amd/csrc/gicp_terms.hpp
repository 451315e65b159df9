// The per-pair terms of K17's linearisation from a symmetric 3 x 3 information matrix M (its upper triangle, row by row) and P = q - c0:
// the 21 entries of H = J^T M J with J = [ -[P]x , I ], one at a time, so that a lane never holds them all (gicp_kernels.hip: the formulas).
// Shared by K17's step kernel and the NDT step kernel (ndt_kernels.hip), which forms the same entries from its weighted sum of matrices.
#pragma once
#include <hip/hip_runtime.h>

namespace mislam {

// entry (i, k) of a symmetric 3 x 3 held as its upper triangle, row by row
__device__ __forceinline__ double sym3(const double (&m)[6], int i, int k)
{
    const int lo = i <= k ? i : k, hi = i <= k ? k : i;
    return m[lo == 0 ? hi : lo + hi + 1];
}

// component a of P x (y0, y1, y2)
__device__ __forceinline__ double cross_at(const double (&P)[3], int a, double y0, double y1, double y2)
{
    return a == 0 ? P[1] * y2 - P[2] * y1 : (a == 1 ? P[2] * y0 - P[0] * y2 : P[0] * y1 - P[1] * y0);
}

__device__ __forceinline__ double gicp_w(const double (&M)[6], const double (&P)[3], int i, int b)
{
    return b < 3 ? cross_at(P, b, sym3(M, i, 0), sym3(M, i, 1), sym3(M, i, 2)) : sym3(M, i, b - 3);
}

__device__ __forceinline__ double gicp_h(const double (&M)[6], const double (&P)[3], int a, int b)
{
    return a < 3 ? cross_at(P, a, gicp_w(M, P, 0, b), gicp_w(M, P, 1, b), gicp_w(M, P, 2, b)) : gicp_w(M, P, a - 3, b);
}

}  // namespace mislam
