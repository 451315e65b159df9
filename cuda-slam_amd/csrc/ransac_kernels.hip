// K23 - K26 hypothesise and verify over correspondences (driver: ransac_api.hip; the contract: mi_ransac_register in mi_slam.h).
//   K23 ransac_hypothesis: one lane per hypothesis.  The three counter-based draws and the edge check in fp64 (ransac_draw.hpp), the Kabsch solve of the three
//                          pairs (fp64 moments rounded to fp32 as solve_from_moments does, kabsch_rotation in the IEEE form, one
//                          Newton-Schulz step in fp64 towards the nearest rotation).  Writes the triple, the valid flag and the fp32 pose.
//   K24 ransac_count:      the hot path, O(H C).  One lane per hypothesis with its pose in registers as fp64; the workgroup stages 256 pairs
//                          at a time in the LDS and every lane reads the same pair at the same time (an LDS broadcast).  Invalid hypotheses
//                          are NOT compacted away first: a lane of an invalid hypothesis walks along with a flag that keeps its count at
//                          zero, which costs its share of the work (the invalid share of a call with Open3D's edge rule is large, so a
//                          stable compaction is the open lever) and keeps h = the lane's index with no indirection.  Where H alone does not
//                          fill the device the pairs are split over gridDim.y and merged by an integer atomicAdd.
//   K25 ransac_argmax:     atomicMax on (inliers << 32 | 0xFFFFFFFF - h) over the valid hypotheses, and their number.
//   K26 ransac_mask / ransac_sum: the inlier flags and fp64 squared distances of every pair under ONE pose, then their count and sum by one
//                          workgroup in a fixed order.
// The refinement's Kabsch over the inliers runs on the kernels behind mi_kabsch.  No floating-point atomics, no scratch.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "ransac_draw.hpp"
#include "svd3.hpp"

namespace mislam {

namespace {

__global__ __launch_bounds__(RANSAC_BLOCK) void ransac_hypothesis_kernel(const RansacHypArgs a)
{
    const int k = blockIdx.x * RANSAC_BLOCK + threadIdx.x;
    if (k >= a.count) return;
    const unsigned long long h = (unsigned long long)(a.first + k);
    unsigned int rank[3];
    for (int r = 0; r < 3; r++) rank[r] = ransac_draw_rank(a.seed, h, r, a.C);      // < C (ransac_draw.hpp)
    float s[3][3], t[3][3];
    for (int r = 0; r < 3; r++) {
        const float* p = a.pairs6 + 6 * (size_t)rank[r];
        for (int d = 0; d < 3; d++) { s[r][d] = p[d]; t[r][d] = p[3 + d]; }
        a.triples[3 * (size_t)k + r] = a.src_index[rank[r]];
    }
    bool valid = rank[0] != rank[1] && rank[0] != rank[2] && rank[1] != rank[2];
    valid = valid && ransac_edges_similar(s, t, a.e2);
    float R9[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}, t3[3] = {0.f, 0.f, 0.f};
    if (valid) {
        // the moments of solve_from_moments (icp_solve.hpp): b = source, a = target; every sum of three left to right
        double cb[3], ca[3];
        for (int d = 0; d < 3; d++) {
            cb[d] = (((double)s[0][d] + (double)s[1][d]) + (double)s[2][d]) * (1.0 / 3.0);
            ca[d] = (((double)t[0][d] + (double)t[1][d]) + (double)t[2][d]) * (1.0 / 3.0);
        }
        Mat3 H;
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++) {
                const double m = ((double)t[0][r] * (double)s[0][c] + (double)t[1][r] * (double)s[1][c]) + (double)t[2][r] * (double)s[2][c];
                H.a[r][c] = (float)(m - 3.0 * ca[r] * cb[c]);
            }
        const Kabsch3 kb = kabsch_rotation<false>(H);                               // the IEEE form, inline
        // The sweeps of the 3 x 3 SVD never re-orthonormalise U and V: over thousands of hypotheses |R^T R - I| reaches 45 eps.  One
        // Newton-Schulz step in fp64, R (1.5 I - 0.5 R^T R), rounded to fp32 once, brings the pose to a rotation within an eps (mi_slam.h)
        double M[3][3];
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) {
                const double g = ((double)kb.R.a[0][i] * (double)kb.R.a[0][j] + (double)kb.R.a[1][i] * (double)kb.R.a[1][j]) + (double)kb.R.a[2][i] * (double)kb.R.a[2][j];
                M[i][j] = (i == j ? 1.5 : 0.0) - 0.5 * g;
            }
        float Ri[9], ti[3];
        for (int c = 0; c < 3; c++)
            for (int r = 0; r < 3; r++)
                Ri[3 * c + r] = (float)(((double)kb.R.a[r][0] * M[0][c] + (double)kb.R.a[r][1] * M[1][c]) + (double)kb.R.a[r][2] * M[2][c]);
        const float fcb[3] = {(float)cb[0], (float)cb[1], (float)cb[2]}, fca[3] = {(float)ca[0], (float)ca[1], (float)ca[2]};
        for (int i = 0; i < 3; i++) ti[i] = fca[i] - ((Ri[i] * fcb[0] + Ri[3 + i] * fcb[1]) + Ri[6 + i] * fcb[2]);
        bool finite = true;
        for (int i = 0; i < 9; i++) finite = finite && (__builtin_fabsf(Ri[i]) <= 3.0e38f);
        for (int i = 0; i < 3; i++) finite = finite && (__builtin_fabsf(ti[i]) <= 3.0e38f);
        valid = finite && kb.S[1] > 0.f;                                            // three collinear points: sigma_2 of H is 0
        if (valid) {
            for (int i = 0; i < 9; i++) R9[i] = Ri[i];
            for (int i = 0; i < 3; i++) t3[i] = ti[i];
        }
    }
    a.valid[k] = valid ? 1 : 0;
    for (int i = 0; i < 9; i++) a.pose12[12 * (size_t)k + i] = R9[i];
    for (int i = 0; i < 3; i++) a.pose12[12 * (size_t)k + 9 + i] = t3[i];
}

// squared distance of pair p6 under the pose (column-major R, t) in fp64, the contract's order
__device__ __forceinline__ double ransac_d2(const double R[9], const double t[3], const float* p6)
{
    const double x = (double)p6[0], y = (double)p6[1], z = (double)p6[2];
    const double dx = (((R[0] * x + R[3] * y) + R[6] * z) + t[0]) - (double)p6[3];
    const double dy = (((R[1] * x + R[4] * y) + R[7] * z) + t[1]) - (double)p6[4];
    const double dz = (((R[2] * x + R[5] * y) + R[8] * z) + t[2]) - (double)p6[5];
    return (dx * dx + dy * dy) + dz * dz;
}

__global__ __launch_bounds__(RANSAC_BLOCK) void ransac_count_kernel(const RansacCountArgs a)
{
    __shared__ float tile[6 * RANSAC_BLOCK];
    const int k = blockIdx.x * RANSAC_BLOCK + threadIdx.x;
    const bool mine = k < a.count;
    double R[9], t[3];
    for (int i = 0; i < 9; i++) R[i] = mine ? (double)a.pose12[12 * (size_t)k + i] : 0.0;
    for (int i = 0; i < 3; i++) t[i] = mine ? (double)a.pose12[12 * (size_t)k + 9 + i] : 0.0;
    const bool valid = mine && a.valid[k] != 0;
    const int begin = blockIdx.y * a.chunk_len, end = min(a.C, begin + a.chunk_len);
    int inliers = 0;
    for (int p0 = begin; p0 < end; p0 += RANSAC_BLOCK) {
        const int rows = min(RANSAC_BLOCK, end - p0);
        __syncthreads();
        for (int e = threadIdx.x; e < 6 * rows; e += RANSAC_BLOCK) tile[e] = a.pairs6[6 * (size_t)p0 + e];
        __syncthreads();
        for (int r = 0; r < rows; r++) inliers += ransac_d2(R, t, tile + 6 * r) <= a.max_d2 ? 1 : 0;
    }
    if (valid && inliers != 0) atomicAdd(&a.inlier_count[k], inliers);
}

__global__ __launch_bounds__(RANSAC_BLOCK) void ransac_argmax_kernel(const unsigned char* valid, const int* inlier_count, int count, unsigned long long* best, int* nvalid)
{
    const int h = blockIdx.x * RANSAC_BLOCK + threadIdx.x;
    if (h >= count || valid[h] == 0) return;
    atomicMax(best, ((unsigned long long)(unsigned int)inlier_count[h] << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned int)h));
    atomicAdd(nvalid, 1);
}

__global__ __launch_bounds__(RANSAC_BLOCK) void ransac_mask_kernel(const RansacMaskArgs a)
{
    const int r = blockIdx.x * RANSAC_BLOCK + threadIdx.x;
    if (r >= a.C) return;
    double R[9], t[3];
    for (int i = 0; i < 9; i++) R[i] = (double)a.pose[i];
    for (int i = 0; i < 3; i++) t[i] = (double)a.pose[9 + i];
    const double d2 = ransac_d2(R, t, a.pairs6 + 6 * (size_t)r);
    const bool in = d2 <= a.max_d2;
    a.mask[r] = in ? 1 : 0;
    a.d2[r] = in ? d2 : 0.0;
}

// out_count[0] = inliers, out_sum[0] = their squared distances: lane l adds ranks l, l + 256, ... in ascending order, then the 256 partial
// sums are added pairwise, stride 128, 64, ... 1 -- one fixed order whatever ran before
__global__ __launch_bounds__(RANSAC_BLOCK) void ransac_sum_kernel(const unsigned char* mask, const double* d2, int C, int* out_count, double* out_sum)
{
    __shared__ double s[RANSAC_BLOCK];
    __shared__ int n[RANSAC_BLOCK];
    double acc = 0.0;
    int cnt = 0;
    for (int r = threadIdx.x; r < C; r += RANSAC_BLOCK) { acc = acc + d2[r]; cnt += mask[r]; }
    s[threadIdx.x] = acc; n[threadIdx.x] = cnt;
    __syncthreads();
    for (int w = RANSAC_BLOCK / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) { s[threadIdx.x] = s[threadIdx.x] + s[threadIdx.x + w]; n[threadIdx.x] += n[threadIdx.x + w]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { out_count[0] = n[0]; out_sum[0] = s[0]; }
}

}  // namespace

hipError_t ransac_hypotheses(const RansacHypArgs& a, hipStream_t s)
{
    if (a.C < 3 || a.first < 0 || a.count < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ransac_hypothesis_kernel, dim3((a.count + RANSAC_BLOCK - 1) / RANSAC_BLOCK), dim3(RANSAC_BLOCK), 0, s, a);
    return hipGetLastError();
}

int ransac_chunk_len(int count, int C, int cu_count)
{
    const long long blocks = ((long long)count + RANSAC_BLOCK - 1) / RANSAC_BLOCK, tiles = ((long long)C + RANSAC_BLOCK - 1) / RANSAC_BLOCK;
    long long chunks = (2LL * cu_count + blocks - 1) / blocks;
    if (chunks < 1) chunks = 1;
    if (chunks > tiles) chunks = tiles;
    if (chunks > 65535) chunks = 65535;
    return (int)((tiles + chunks - 1) / chunks) * RANSAC_BLOCK;
}

hipError_t ransac_count(const RansacCountArgs& a, hipStream_t s)
{
    if (a.C < 1 || a.count < 1 || a.chunk_len < RANSAC_BLOCK || a.chunk_len % RANSAC_BLOCK != 0) return hipErrorInvalidValue;
    const long long chunks = ((long long)a.C + a.chunk_len - 1) / a.chunk_len;
    if (chunks > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ransac_count_kernel, dim3((a.count + RANSAC_BLOCK - 1) / RANSAC_BLOCK, (unsigned int)chunks), dim3(RANSAC_BLOCK), 0, s, a);
    return hipGetLastError();
}

hipError_t ransac_argmax(const unsigned char* valid, const int* inlier_count, int count, unsigned long long* best, int* nvalid, hipStream_t s)
{
    if (count < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ransac_argmax_kernel, dim3((count + RANSAC_BLOCK - 1) / RANSAC_BLOCK), dim3(RANSAC_BLOCK), 0, s, valid, inlier_count, count, best, nvalid);
    return hipGetLastError();
}

hipError_t ransac_mask_and_sum(const RansacMaskArgs& a, int* out_count, double* out_sum, hipStream_t s)
{
    if (a.C < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ransac_mask_kernel, dim3((a.C + RANSAC_BLOCK - 1) / RANSAC_BLOCK), dim3(RANSAC_BLOCK), 0, s, a);
    hipLaunchKernelGGL(ransac_sum_kernel, dim3(1), dim3(RANSAC_BLOCK), 0, s, a.mask, a.d2, a.C, out_count, out_sum);
    return hipGetLastError();
}

// loads this translation unit's code object at mi_ctx_preload (kernels.h)
__global__ void preload_ransac_kernels_kernel() {}
hipError_t preload_ransac_kernels()
{
    hipFuncAttributes attr;
    return hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(preload_ransac_kernels_kernel));
}

}  // namespace mislam
