// The counter-based draws and the edge rule of mi_ransac_register (the contract: mi_slam.h), stated once for K23 (ransac_kernels.hip) and for
// the tuple filter of mi_fgr_register (K44, fgr_kernels.hip): a trial needs no state, so any lane can form any trial.
#pragma once
#include <hip/hip_runtime.h>

namespace mislam {

__device__ __forceinline__ unsigned long long ransac_mix(unsigned long long z)     // the splitmix64 finaliser
{
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}

// draw r (0, 1, 2) of hypothesis h among C correspondences: a rank < C
__device__ __forceinline__ unsigned int ransac_draw_rank(unsigned long long seed, unsigned long long h, int r, int C)
{
    const unsigned long long u = ransac_mix(seed + 0x9E3779B97F4A7C15ull * (3ull * h + (unsigned long long)r + 1ull));
    return (unsigned int)(((u >> 32) * (unsigned long long)C) >> 32);
}

__device__ __forceinline__ double ransac_len2(const float* p, const float* q)
{
    const double x = (double)p[0] - (double)q[0], y = (double)p[1] - (double)q[1], z = (double)p[2] - (double)q[2];
    return (x * x + y * y) + z * z;
}

// the edges (0, 1), (1, 2), (0, 2) of three source points s and their three target points t, written out: constant indices keep the
// points in registers
__device__ __forceinline__ bool ransac_edges_similar(const float (&s)[3][3], const float (&t)[3][3], double e2)
{
    const double ls01 = ransac_len2(s[0], s[1]), lt01 = ransac_len2(t[0], t[1]);
    const double ls12 = ransac_len2(s[1], s[2]), lt12 = ransac_len2(t[1], t[2]);
    const double ls02 = ransac_len2(s[0], s[2]), lt02 = ransac_len2(t[0], t[2]);
    return ls01 >= e2 * lt01 && lt01 >= e2 * ls01 && ls12 >= e2 * lt12 && lt12 >= e2 * ls12 && ls02 >= e2 * lt02 && lt02 >= e2 * ls02;
}

}  // namespace mislam
