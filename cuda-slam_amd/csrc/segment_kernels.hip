// K39 - K43 the dominant planes of a cloud (driver: segment_api.hip; the contract: mi_segment_plane in mi_slam.h).  K23 - K26's pattern
// (ransac_kernels.hip) over the REMAINING points of a round instead of correspondences:
//   K39 segment_hypothesis: one lane per hypothesis.  The three counter-based draws with the global number g = round * H + h, the cross
//                           product and its normalisation in fp64, the plane rounded to fp32, the axis rule.  Writes the triple (the
//                           caller's indices), the valid flag and the fp32 plane.
//   K40 segment_count:      the hot path, O(H C).  One lane per hypothesis with its plane and T2 nn in registers as fp64.  The workgroup
//                           stages 256 points at a time in the LDS AS fp64 (each coordinate converted once per tile, by the lane that
//                           stages it, instead of once per lane and point) and every lane reads the same point at the same time, a
//                           broadcast; a lane takes TWO points per trip, 48 contiguous bytes on a 16-byte boundary (three 16-byte reads).
//                           A tile with an odd number of rows gets one NaN point behind its last: it fails every comparison.  Invalid
//                           hypotheses walk along and add nothing (h = the lane's index, as K24).  Where H alone does not fill the
//                           device the points are split over gridDim.y and merged by an integer atomicAdd.
//   K41 segment_mask:       the inlier flags and fp64 s s / nn of every remaining point under ONE plane.
//   K42 segment_sum / segment_scatter: one workgroup each, ransac_sum's fixed order -- the count, S and the coordinate sums of the inliers;
//                           then the six sums of products about the centroid those give.
//   K43 segment_begin / segment_label: labels = -1 and keep = 1 for a call; a plane's number and keep = 0 at its inliers.
// The winner is ransac_argmax's (K25), the peel outlier_compact's (K15).  No floating-point atomics, no scratch.
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace mislam {

namespace {

__device__ __forceinline__ unsigned long long segment_mix(unsigned long long z)    // the splitmix64 finaliser
{
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}

__device__ __forceinline__ bool segment_finite(float v) { return __builtin_fabsf(v) < __builtin_inff(); }   // (false for NaN)

__global__ __launch_bounds__(SEGMENT_BLOCK) void segment_hypothesis_kernel(const SegmentHypArgs a)
{
    const int k = blockIdx.x * SEGMENT_BLOCK + threadIdx.x;
    if (k >= a.count) return;
    const unsigned long long g = a.g0 + (unsigned long long)k;
    unsigned int rank[3];
    for (int r = 0; r < 3; r++) {
        const unsigned long long u = segment_mix(a.seed + 0x9E3779B97F4A7C15ull * (3ull * g + (unsigned long long)r + 1ull));
        rank[r] = (unsigned int)(((u >> 32) * (unsigned long long)a.C) >> 32);      // < C
    }
    double p[3][3];
    for (int r = 0; r < 3; r++) {
        const float* q = a.rem_xyz + 3 * (size_t)rank[r];
        for (int d = 0; d < 3; d++) p[r][d] = (double)q[d];
        a.triples[3 * (size_t)k + r] = a.rem_index[rank[r]];
    }
    bool valid = rank[0] != rank[1] && rank[0] != rank[2] && rank[1] != rank[2];
    const double e1x = p[1][0] - p[0][0], e1y = p[1][1] - p[0][1], e1z = p[1][2] - p[0][2];
    const double e2x = p[2][0] - p[0][0], e2y = p[2][1] - p[0][1], e2z = p[2][2] - p[0][2];
    const double Nx = e1y * e2z - e1z * e2y, Ny = e1z * e2x - e1x * e2z, Nz = e1x * e2y - e1y * e2x;
    const double len2 = (Nx * Nx + Ny * Ny) + Nz * Nz;
    valid = valid && len2 > 0.0 && len2 < (double)__builtin_inff();                 // (false for NaN)
    float pl[4] = {0.f, 0.f, 0.f, 0.f};
    if (valid) {
        const double q = 1.0 / sqrt(len2);
        const float fa = (float)(Nx * q), fb = (float)(Ny * q), fc = (float)(Nz * q);
        const float fd = (float)(-(((Nx * p[0][0] + Ny * p[0][1]) + Nz * p[0][2]) * q));
        valid = segment_finite(fa) && segment_finite(fb) && segment_finite(fc) && segment_finite(fd);
        if (valid && a.has_axis) {
            const double da = (double)fa, db = (double)fb, dc = (double)fc;
            const double dot = (da * a.axis[0] + db * a.axis[1]) + dc * a.axis[2];
            const double aa = (a.axis[0] * a.axis[0] + a.axis[1] * a.axis[1]) + a.axis[2] * a.axis[2];
            const double nn = (da * da + db * db) + dc * dc;
            valid = dot * dot >= a.cos2 * (aa * nn);
        }
        if (valid) { pl[0] = fa; pl[1] = fb; pl[2] = fc; pl[3] = fd; }
    }
    a.valid[k] = valid ? 1 : 0;
    for (int i = 0; i < 4; i++) a.plane4[4 * (size_t)k + i] = pl[i];
}

__global__ __launch_bounds__(SEGMENT_BLOCK) void segment_count_kernel(const SegmentCountArgs a)
{
    __shared__ __align__(16) double tile[3 * SEGMENT_BLOCK];
    const int k = blockIdx.x * SEGMENT_BLOCK + threadIdx.x;
    const bool mine = k < a.count;
    double pa = 0.0, pb = 0.0, pc = 0.0, pd = 0.0;
    if (mine) {
        pa = (double)a.plane4[4 * (size_t)k]; pb = (double)a.plane4[4 * (size_t)k + 1];
        pc = (double)a.plane4[4 * (size_t)k + 2]; pd = (double)a.plane4[4 * (size_t)k + 3];
    }
    const double t2nn = a.T2 * ((pa * pa + pb * pb) + pc * pc);
    const bool valid = mine && a.valid[k] != 0;
    const int begin = blockIdx.y * a.chunk_len, end = min(a.C, begin + a.chunk_len);
    int inliers = 0;
    for (int p0 = begin; p0 < end; p0 += SEGMENT_BLOCK) {
        const int rows = min(SEGMENT_BLOCK, end - p0);
        const int padded = (rows + 1) & ~1;                                         // <= SEGMENT_BLOCK, which is even
        __syncthreads();
        for (int e = threadIdx.x; e < 3 * padded; e += SEGMENT_BLOCK)
            tile[e] = e < 3 * rows ? (double)a.rem_xyz[3 * (size_t)p0 + e] : (double)__builtin_nanf("");
        __syncthreads();
        for (int r = 0; r < padded; r += 2) {
            const double* t = tile + 3 * r;
            const double s0 = ((pa * t[0] + pb * t[1]) + pc * t[2]) + pd;
            const double s1 = ((pa * t[3] + pb * t[4]) + pc * t[5]) + pd;
            inliers += s0 * s0 <= t2nn ? 1 : 0;
            inliers += s1 * s1 <= t2nn ? 1 : 0;
        }
    }
    if (valid && inliers != 0) atomicAdd(&a.inlier_count[k], inliers);
}

__global__ __launch_bounds__(SEGMENT_BLOCK) void segment_mask_kernel(const SegmentMaskArgs a)
{
    const int r = blockIdx.x * SEGMENT_BLOCK + threadIdx.x;
    if (r >= a.C) return;
    const double pa = (double)a.plane[0], pb = (double)a.plane[1], pc = (double)a.plane[2], pd = (double)a.plane[3];
    const double nn = (pa * pa + pb * pb) + pc * pc;
    const float* q = a.rem_xyz + 3 * (size_t)r;
    const double s = ((pa * (double)q[0] + pb * (double)q[1]) + pc * (double)q[2]) + pd;
    const bool in = s * s <= a.T2 * nn;
    a.mask[r] = in ? 1 : 0;
    a.s2[r] = in ? (s * s) / nn : 0.0;
}

// NV fp64 sums and a count over one workgroup, ransac_sum's order: lane l adds ranks l, l + 256, ... in ascending order, then the 256
// partial sums are added pairwise, stride 128, 64, ... 1.  Behind it thread 0 holds the results in acc[] and cnt.
template <int NV>
__device__ __forceinline__ void segment_fold(double (&acc)[NV], int& cnt)
{
    __shared__ double s[NV][SEGMENT_BLOCK];
    __shared__ int n[SEGMENT_BLOCK];
#pragma unroll
    for (int v = 0; v < NV; v++) s[v][threadIdx.x] = acc[v];
    n[threadIdx.x] = cnt;
    __syncthreads();
    for (int w = SEGMENT_BLOCK / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
#pragma unroll
            for (int v = 0; v < NV; v++) s[v][threadIdx.x] = s[v][threadIdx.x] + s[v][threadIdx.x + w];
            n[threadIdx.x] += n[threadIdx.x + w];
        }
        __syncthreads();
    }
#pragma unroll
    for (int v = 0; v < NV; v++) acc[v] = s[v][0];
    cnt = n[0];
}

// sums[0] = the inliers' number, sums[1] = S, sums[2 .. 4] = their coordinate sums
__global__ __launch_bounds__(SEGMENT_BLOCK) void segment_sum_kernel(const SegmentMaskArgs a)
{
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    int cnt = 0;
    for (int r = threadIdx.x; r < a.C; r += SEGMENT_BLOCK) {
        const bool in = a.mask[r] != 0;
        const float* q = a.rem_xyz + 3 * (size_t)r;
        acc[0] = acc[0] + a.s2[r];
        acc[1] = acc[1] + (in ? (double)q[0] : 0.0);
        acc[2] = acc[2] + (in ? (double)q[1] : 0.0);
        acc[3] = acc[3] + (in ? (double)q[2] : 0.0);
        cnt += in ? 1 : 0;
    }
    segment_fold<4>(acc, cnt);
    if (threadIdx.x == 0) {
        a.sums[0] = (double)cnt;
        for (int v = 0; v < 4; v++) a.sums[1 + v] = acc[v];
    }
}

// sums[5 .. 10] = xx xy xz yy yz zz of (p - centroid) over the inliers, centroid = sums[2 .. 4] / sums[0]; sums[11] = 0
__global__ __launch_bounds__(SEGMENT_BLOCK) void segment_scatter_kernel(const SegmentMaskArgs a)
{
    const double count = a.sums[0];
    const bool any = count >= 1.0;
    const double cx = any ? a.sums[2] / count : 0.0, cy = any ? a.sums[3] / count : 0.0, cz = any ? a.sums[4] / count : 0.0;
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    int cnt = 0;
    for (int r = threadIdx.x; r < a.C; r += SEGMENT_BLOCK) {
        const bool in = a.mask[r] != 0;
        const float* q = a.rem_xyz + 3 * (size_t)r;
        const double dx = (double)q[0] - cx, dy = (double)q[1] - cy, dz = (double)q[2] - cz;
        acc[0] = acc[0] + (in ? dx * dx : 0.0);
        acc[1] = acc[1] + (in ? dx * dy : 0.0);
        acc[2] = acc[2] + (in ? dx * dz : 0.0);
        acc[3] = acc[3] + (in ? dy * dy : 0.0);
        acc[4] = acc[4] + (in ? dy * dz : 0.0);
        acc[5] = acc[5] + (in ? dz * dz : 0.0);
    }
    segment_fold<6>(acc, cnt);
    if (threadIdx.x == 0) {
        for (int v = 0; v < 6; v++) a.sums[5 + v] = acc[v];
        a.sums[11] = 0.0;
    }
}

__global__ __launch_bounds__(SEGMENT_BLOCK) void segment_begin_kernel(int* __restrict__ labels, unsigned char* __restrict__ keep, int n)
{
    const int i = blockIdx.x * SEGMENT_BLOCK + threadIdx.x;
    if (i >= n) return;
    labels[i] = -1;
    keep[i] = 1;
}

__global__ __launch_bounds__(SEGMENT_BLOCK) void segment_label_kernel(const unsigned char* __restrict__ mask, const int* __restrict__ rem_index, int C, int plane,
                                                                      int* __restrict__ labels, unsigned char* __restrict__ keep)
{
    const int r = blockIdx.x * SEGMENT_BLOCK + threadIdx.x;
    if (r >= C || mask[r] == 0) return;
    const int i = rem_index[r];
    labels[i] = plane;
    keep[i] = 0;
}

inline unsigned int segment_blocks(int n) { return (unsigned int)(((long long)n + SEGMENT_BLOCK - 1) / SEGMENT_BLOCK); }

}  // namespace

hipError_t segment_hypotheses(const SegmentHypArgs& a, hipStream_t s)
{
    if (a.C < 3 || a.count < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(segment_hypothesis_kernel, dim3(segment_blocks(a.count)), dim3(SEGMENT_BLOCK), 0, s, a);
    return hipGetLastError();
}

hipError_t segment_count(const SegmentCountArgs& a, hipStream_t s)
{
    if (a.C < 1 || a.count < 1 || a.chunk_len < SEGMENT_BLOCK || a.chunk_len % SEGMENT_BLOCK != 0) return hipErrorInvalidValue;
    const long long chunks = ((long long)a.C + a.chunk_len - 1) / a.chunk_len;
    if (chunks > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(segment_count_kernel, dim3(segment_blocks(a.count), (unsigned int)chunks), dim3(SEGMENT_BLOCK), 0, s, a);
    return hipGetLastError();
}

hipError_t segment_mask_and_sums(const SegmentMaskArgs& a, int want_scatter, hipStream_t s)
{
    if (a.C < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(segment_mask_kernel, dim3(segment_blocks(a.C)), dim3(SEGMENT_BLOCK), 0, s, a);
    hipLaunchKernelGGL(segment_sum_kernel, dim3(1), dim3(SEGMENT_BLOCK), 0, s, a);
    if (want_scatter) hipLaunchKernelGGL(segment_scatter_kernel, dim3(1), dim3(SEGMENT_BLOCK), 0, s, a);
    return hipGetLastError();
}

hipError_t segment_begin(int* labels, unsigned char* keep, int n, hipStream_t s)
{
    if (n < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(segment_begin_kernel, dim3(segment_blocks(n)), dim3(SEGMENT_BLOCK), 0, s, labels, keep, n);
    return hipGetLastError();
}

hipError_t segment_label(const unsigned char* mask, const int* rem_index, int C, int plane, int* labels, unsigned char* keep, hipStream_t s)
{
    if (C < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(segment_label_kernel, dim3(segment_blocks(C)), dim3(SEGMENT_BLOCK), 0, s, mask, rem_index, C, plane, labels, keep);
    return hipGetLastError();
}

// loads this translation unit's code object at mi_ctx_preload (kernels.h)
__global__ void preload_segment_kernels_kernel() {}
hipError_t preload_segment_kernels()
{
    hipFuncAttributes attr;
    return hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(preload_segment_kernels_kernel));
}

}  // namespace mislam
