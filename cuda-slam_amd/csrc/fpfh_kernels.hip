// K18 / K19 -- Fast Point Feature Histograms of a cloud with normals (mi_fpfh_features; driver: fpfh_api.hip; the contract: mi_slam.h).
//
// K18, SPFH: one lane per point.  The search is K13's in self mode, the body of knn_scan.hpp: after it the lane holds its point's
//   neighbourhood as K sorted keys in registers -- the same keys, bit for bit, that mi_knn_search would have written out.
//   keys     the k-list goes to memory as it is (n x k keys): the second pass reads it and does not search again.
//   pairs    the list is then consumed from its far end: the last register is the pair to work on, and the list moves up by one -- K
//            register moves with static indices per trip, so the loop over the k slots stays a loop (one copy of the pair arithmetic and
//            its atan2 in the code, not K of them) and no index into the list is computed at run time.  The counts are integers: the
//            order in which the pairs are taken does not show in them.  The neighbour's point and normal come from the SoA arrays in the
//            caller's order; the features and bins are fpfh_pair.hpp's, in fp64.
//   counts   a count is at most 32, so the 11 bins of a feature are bytes of three 32-bit words, nine words for the three features; the
//            bin picks one of three words and a shift, with selects -- no array is indexed by the bin, nothing goes to scratch.  The
//            spare byte of every feature's third word holds the point's neighbour count.  Those nine words, 36 bytes per point, are
//            what the second pass gathers.
// K19, FPFH: three lanes per point, one feature each, along the curve order of K18 (neighbours of neighbouring lanes are near in
//   memory).  A lane walks its point's keys in key order, and for every neighbour at d2 > 0 gathers the three words of its feature
//   (they carry the neighbour's count) and adds s_b(j) / d2 to its 11 fp64 sums and to the feature's total, b ascending: the order of
//   the contract, whatever the layout.  Then the scale, the point's own SPFH, one rounding to fp32, 11 floats out.
// No LDS, no atomics, no scratch in either kernel.
#include <hip/hip_runtime.h>

#include "fpfh_pair.hpp"
#include "kernels.h"
#include "knn_scan.hpp"
#include "nn_grid.h"

namespace mislam {

static_assert(FPFH_WORDS == 3 * ((FPFH_BINS + 3) / 4) && FPFH_DIM == 3 * FPFH_BINS, "nine words: three per feature, four bins a word");
static_assert(KNN_MAX_K <= 255, "a count fits a byte");

namespace {

// one more pair in bin b (0 .. 10) of a feature's three words
__device__ __forceinline__ void fpfh_count_bin(unsigned int& w0, unsigned int& w1, unsigned int& w2, int b)
{
    const unsigned int one = 1u << ((b & 3) * 8);
    const int word = b >> 2;
    w0 += word == 0 ? one : 0u;
    w1 += word == 1 ? one : 0u;
    w2 += word == 2 ? one : 0u;
}

// the count of bin B (static) of a feature's three words
template <int B>
__device__ __forceinline__ unsigned int fpfh_bin_count(unsigned int w0, unsigned int w1, unsigned int w2)
{
    const unsigned int w = B < 4 ? w0 : (B < 8 ? w1 : w2);
    return (w >> ((B & 3) * 8)) & 0xffu;
}

template <int K, bool FMA>
__global__ __launch_bounds__(KNN_BLOCK) void fpfh_spfh_kernel(NnGridView g, FpfhSpfhArgs a)
{
    const int s = blockIdx.x * KNN_BLOCK + (int)threadIdx.x;
    if (s >= a.q.n) return;
    const float q[3] = {a.q.x[s], a.q.y[s], a.q.z[s]};
    const int row_out = a.q.order[s];
    const int k = a.k;

    unsigned long long l[K];
#pragma unroll
    for (int i = 0; i < K; i++) l[i] = i < K - k ? 0ull : KNN_KEY_EMPTY;
    knn_scan<K, FMA>(g, q, a.q.hi, (unsigned int)row_out, k, a.max_d2, l);

    unsigned long long* keys = a.keys + (size_t)row_out * (size_t)k;
#pragma unroll
    for (int i = 0; i < K; i++) {
        const int slot = i - (K - k);
        if (slot >= 0) keys[slot] = l[i];
    }

    const double pix = (double)q[0], piy = (double)q[1], piz = (double)q[2];
    const double nix = (double)a.nx[row_out], niy = (double)a.ny[row_out], niz = (double)a.nz[row_out];
    unsigned int t0 = 0u, t1 = 0u, t2 = 0u, a0 = 0u, a1 = 0u, a2 = 0u, p0 = 0u, p1 = 0u, p2 = 0u;
    unsigned int found = 0u;
#pragma unroll 1
    for (int trip = 0; trip < k; trip++) {
        const unsigned long long key = l[K - 1];
#pragma unroll
        for (int i = K - 1; i >= 1; i--) l[i] = l[i - 1];
        if ((unsigned int)(key >> 32) < 0x7f800000u) {                             // a filled slot of the k-list
            const unsigned int j = (unsigned int)(key & 0xffffffffull);            // (< n: the index the grid build stored)
            double theta, alpha, phi;
            fpfh_pair_features(pix, piy, piz, nix, niy, niz, (double)a.c.x[j], (double)a.c.y[j], (double)a.c.z[j], (double)a.nx[j], (double)a.ny[j],
                               (double)a.nz[j], theta, alpha, phi);
            fpfh_count_bin(t0, t1, t2, fpfh_bin_angle(theta));
            fpfh_count_bin(a0, a1, a2, fpfh_bin_cosine(alpha));
            fpfh_count_bin(p0, p1, p2, fpfh_bin_cosine(phi));
            found++;
        }
    }
    unsigned int* out = a.packed + (size_t)FPFH_WORDS * (size_t)row_out;
    out[0] = t0; out[1] = t1; out[2] = t2 | (found << 24);
    out[3] = a0; out[4] = a1; out[5] = a2 | (found << 24);
    out[6] = p0; out[7] = p1; out[8] = p2 | (found << 24);
    if (a.count) a.count[row_out] = (int)found;
}

// s_b = (100 c_b) / count as a value, 0 for a point without neighbours
__device__ __forceinline__ double fpfh_spfh_value(unsigned int c, unsigned int count, double count_d)
{
    return count != 0u ? (100.0 * (double)c) / count_d : 0.0;
}

template <int B>
__device__ __forceinline__ void fpfh_add_neighbour(double (&F)[FPFH_BINS], double& S, unsigned int w0, unsigned int w1, unsigned int w2, unsigned int count,
                                                   double count_d, double d2)
{
    const double val = fpfh_spfh_value(fpfh_bin_count<B>(w0, w1, w2), count, count_d) / d2;
    F[B] += val;
    S += val;
    if constexpr (B + 1 < FPFH_BINS) fpfh_add_neighbour<B + 1>(F, S, w0, w1, w2, count, count_d, d2);
}

template <int B>
__device__ __forceinline__ void fpfh_finish(const double (&F)[FPFH_BINS], double scale, unsigned int w0, unsigned int w1, unsigned int w2, unsigned int count,
                                            double count_d, float* out, unsigned char* counts)
{
    const unsigned int c = fpfh_bin_count<B>(w0, w1, w2);
    out[B] = (float)(F[B] * scale + fpfh_spfh_value(c, count, count_d));
    if (counts) counts[B] = (unsigned char)c;
    if constexpr (B + 1 < FPFH_BINS) fpfh_finish<B + 1>(F, scale, w0, w1, w2, count, count_d, out, counts);
}

__global__ __launch_bounds__(FPFH_SUM_BLOCK) void fpfh_sum_kernel(FpfhSumArgs a)
{
    const int s = blockIdx.x * FPFH_SUM_POINTS + (int)threadIdx.x / 3;
    const int f = (int)threadIdx.x % 3;                                             // the lane's feature: theta, alpha, phi
    if (s >= a.n) return;
    const size_t row = (size_t)a.order[s];
    const unsigned int* own = a.packed + FPFH_WORDS * row + 3 * f;
    const unsigned int o0 = own[0], o1 = own[1], o2 = own[2];
    const unsigned int count = o2 >> 24;

    double F[FPFH_BINS];
#pragma unroll
    for (int b = 0; b < FPFH_BINS; b++) F[b] = 0.0;
    double S = 0.0;
    const unsigned long long* keys = a.keys + row * (size_t)a.k;
    for (unsigned int r = 0; r < count; r++) {                                      // the filled slots come first, nearest first
        const unsigned long long key = keys[r];
        const float d2 = __uint_as_float((unsigned int)(key >> 32));
        if (!(d2 > 0.f)) continue;                                                  // a duplicate is no weight
        const unsigned int* nb = a.packed + FPFH_WORDS * (size_t)(unsigned int)(key & 0xffffffffull) + 3 * f;
        const unsigned int w0 = nb[0], w1 = nb[1], w2 = nb[2];
        const unsigned int nc = w2 >> 24;
        fpfh_add_neighbour<0>(F, S, w0, w1, w2, nc, (double)nc, (double)d2);
    }
    const double scale = S != 0.0 ? 100.0 / S : 0.0;
    fpfh_finish<0>(F, scale, o0, o1, o2, count, (double)count, a.fpfh + FPFH_DIM * row + FPFH_BINS * f,
                   a.counts ? a.counts + FPFH_DIM * row + FPFH_BINS * f : nullptr);
}

}  // namespace

hipError_t fpfh_spfh(const NnGridView& g, const FpfhSpfhArgs& a, int fma, hipStream_t s)
{
    if (a.q.n < 1 || a.k < 1 || a.k > KNN_MAX_K) return hipErrorInvalidValue;
    knn_dispatch(a.q.n, a.k, fma, [&](auto list, auto fused, dim3 grid) {
        hipLaunchKernelGGL((fpfh_spfh_kernel<decltype(list)::value, decltype(fused)::value>), grid, dim3(KNN_BLOCK), 0, s, g, a);
    });
    return hipGetLastError();
}

hipError_t fpfh_sum(const FpfhSumArgs& a, hipStream_t s)
{
    if (a.n < 1 || a.k < 1 || a.k > KNN_MAX_K) return hipErrorInvalidValue;
    const dim3 grid((a.n + FPFH_SUM_POINTS - 1) / FPFH_SUM_POINTS);
    hipLaunchKernelGGL(fpfh_sum_kernel, grid, dim3(FPFH_SUM_BLOCK), 0, s, a);
    return hipGetLastError();
}

// loads this translation unit's code object at mi_ctx_preload (kernels.h)
__global__ void preload_fpfh_kernels_kernel() {}
hipError_t preload_fpfh_kernels()
{
    hipFuncAttributes attr;
    return hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(preload_fpfh_kernels_kernel));
}

}  // namespace mislam
