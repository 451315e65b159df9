// The range pass every cloud-taking call opens with: per-axis minimum and maximum of a cloud and, where the call refuses points, the lowest
// index of a refused one.  Two stages, like reduce.hpp: per-lane accumulators -> LDS halving tree -> one partial row per block; one
// workgroup of 256 lanes then folds the rows and its thread 0 runs the caller's epilogue.  Stated once here; a caller supplies how a point
// is loaded, which points it refuses, its block cap, and the epilogue (nn_tree.hip, knn_kernels.hip, voxel_kernels.hip, prepare_api.hip,
// and mi_selftest_cloud_range, which runs nothing else).
//
// Bits.  Every result is a minimum or a maximum, hence one of the inputs, and does not depend on the order of the fold -- two corners:
//   NaN           fminf / fmaxf drop a NaN operand (v_min_f32 / v_max_f32 in IEEE mode return the other one), so a pass that refuses
//                 nothing IGNORES NaN coordinates; an axis with nothing but NaNs stays at +inf / -inf.
//   signed zeros  the fold relies on v_min_f32 ordering -0 below +0 and v_max_f32 +0 above -0 in either operand order (the CDNA ISA's
//                 definition of the two instructions; fminf / fmaxf compile to them), so that an axis whose extreme is zero reports one
//                 sign bit for every order of the fold.  tests/test_gpu_cloud_range.py checks it on the device: a cloud against its reversal.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace mislam {

constexpr int RANGE_NO_POINT = 0x7fffffff;   // "no point refused" (= KNN_NO_POINT = VOX_NO_POINT)
static_assert(KNN_NO_POINT == RANGE_NO_POINT && VOX_NO_POINT == RANGE_NO_POINT, "one value for 'no point refused'");

// ---- predicates: is the point usable?  REFUSES = false: the pass carries no bad index at all
struct AnyPoint {
    static constexpr bool REFUSES = false;
    __device__ __forceinline__ bool operator()(float, float, float) const { return true; }
};
struct FinitePoint {      // finite3
    static constexpr bool REFUSES = true;
    __device__ __forceinline__ bool operator()(float x, float y, float z) const
    {
        return fabsf(x) < __builtin_inff() && fabsf(y) < __builtin_inff() && fabsf(z) < __builtin_inff();     // (false for NaN)
    }
};
struct UsablePoint {      // usable3
    static constexpr bool REFUSES = true;
    __device__ __forceinline__ bool operator()(float x, float y, float z) const
    {
        return fabsf(x) <= KNN_MAX_COORD && fabsf(y) <= KNN_MAX_COORD && fabsf(z) <= KNN_MAX_COORD;     // (false for NaN and the infinities)
    }
};

// ---- loader of a SoA cloud
struct SoaPoints {
    const float *__restrict__ x, *__restrict__ y, *__restrict__ z;
    __device__ __forceinline__ void operator()(int i, float (&p)[3]) const { p[0] = x[i]; p[1] = y[i]; p[2] = z[i]; }
};

// what a lane carries: lo xyz, hi xyz, and the lowest refused index of up to two checked arrays (slots a pass does not use cost nothing)
struct RangeAcc {
    float v[6];
    int bad[2];
};
__device__ __forceinline__ void range_clear(RangeAcc& a)
{
#pragma unroll
    for (int k = 0; k < 6; k++) a.v[k] = k < 3 ? __builtin_inff() : -__builtin_inff();
    a.bad[0] = a.bad[1] = RANGE_NO_POINT;
}

// The halving tree over the block's 256 lanes: six floats and NBAD indices.  Behind it, column 0 of the LDS rows holds the result.
struct RangeLds {
    const float (*s)[256];
    const int (*sb)[256];
};
template <int NBAD>
__device__ __forceinline__ RangeLds range_fold(const RangeAcc& a)
{
    __shared__ float s[6][256];
    int(*sb)[256] = nullptr;
    if constexpr (NBAD > 0) {
        __shared__ int bad_rows[NBAD][256];
        sb = bad_rows;
    }
    const int t = threadIdx.x;
#pragma unroll
    for (int k = 0; k < 6; k++) s[k][t] = a.v[k];
#pragma unroll
    for (int j = 0; j < NBAD; j++) sb[j][t] = a.bad[j];
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (t < w) {
#pragma unroll
            for (int k = 0; k < 6; k++) s[k][t] = k < 3 ? fminf(s[k][t], s[k][t + w]) : fmaxf(s[k][t], s[k][t + w]);
#pragma unroll
            for (int j = 0; j < NBAD; j++) sb[j][t] = min(sb[j][t], sb[j][t + w]);
        }
        __syncthreads();
    }
    return RangeLds{s, sb};
}

// The per-block part: grid-stride loop over n points, tree, the block's row -> lo_hi[blockIdx.x][6] (and bad[blockIdx.x] when the predicate
// can refuse; else `bad` is not touched and may be null).  A refused point contributes min(first_bad, i) and nothing else.
template <class Load, class Pred>
__device__ __forceinline__ void range_block(const Load& load, const Pred& usable, int n, float* __restrict__ lo_hi, int* __restrict__ bad)
{
    RangeAcc a;
    range_clear(a);
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        float p[3];
        load(i, p);
        if (Pred::REFUSES && !usable(p[0], p[1], p[2])) { a.bad[0] = min(a.bad[0], i); continue; }
#pragma unroll
        for (int k = 0; k < 3; k++) { a.v[k] = fminf(a.v[k], p[k]); a.v[3 + k] = fmaxf(a.v[3 + k], p[k]); }
    }
    const RangeLds f = range_fold<Pred::REFUSES ? 1 : 0>(a);
    if (threadIdx.x < 6) lo_hi[blockIdx.x * 6 + threadIdx.x] = f.s[threadIdx.x][0];
    if (Pred::REFUSES && threadIdx.x == 0) bad[blockIdx.x] = f.sb[0][0];
}

// The finish part: 256 lanes fold nblocks partial rows (NBAD >= 1: and their bad indices; NBAD == 2: and nblocks2 bad indices of a second
// array, which brings no rows).  True in thread 0 alone, where `a` then holds the result and the caller's epilogue runs.
template <int NBAD>
__device__ __forceinline__ bool range_finish(RangeAcc& a, const float* __restrict__ lo_hi, int nblocks, const int* __restrict__ bad = nullptr,
                                             const int* __restrict__ bad2 = nullptr, int nblocks2 = 0)
{
    range_clear(a);
    for (int b = threadIdx.x; b < nblocks; b += 256) {
#pragma unroll
        for (int k = 0; k < 6; k++) a.v[k] = k < 3 ? fminf(a.v[k], lo_hi[b * 6 + k]) : fmaxf(a.v[k], lo_hi[b * 6 + k]);
        if (NBAD >= 1) a.bad[0] = min(a.bad[0], bad[b]);
    }
    if (NBAD >= 2)
        for (int b = threadIdx.x; b < nblocks2; b += 256) a.bad[1] = min(a.bad[1], bad2[b]);
    const RangeLds f = range_fold<NBAD>(a);
    if (threadIdx.x != 0) return false;
#pragma unroll
    for (int k = 0; k < 6; k++) a.v[k] = f.s[k][0];
#pragma unroll
    for (int j = 0; j < NBAD; j++) a.bad[j] = f.sb[j][0];
    return true;
}

// blocks of the per-block part for n points under the caller's cap (= partial rows the finish folds)
inline int range_blocks(int n, int cap)
{
    const int nb = (n + 255) / 256;
    return nb < 1 ? 1 : (nb < cap ? nb : cap);
}

}  // namespace mislam
