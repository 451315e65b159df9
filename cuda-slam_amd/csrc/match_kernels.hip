// K20 / K21 descriptor matching (driver: match_api.hip; the contract: mi_feature_match in mi_slam.h).
//   K20 match_norms: one lane per row.  The row's norm as the contract's fmaf chain and the input check (lowest refused row by atomicMin).
//   K21 match_mfma:  every pair's dot product on the matrix pipe, v_mfma_f32_32x32x2_f32, which is bit for bit the contract's k-ordered
//                    fmaf chain.  A workgroup of four waves owns 128 rows of the side that searches ("queries") and streams tiles of 128 rows
//                    of the side that is searched ("targets") of its chunk through the LDS.  The TARGETS are the instruction's A operand and
//                    the queries its B operand, so that an accumulator's column -- the lane -- is a query and its 16 registers are 16 targets
//                    in ascending order: the running (key, index) minimum of a query is kept in two registers of its lane, no lane talks to
//                    another until the two halves of the wave (targets 4 h + ... of every group of eight) are merged once at the end.
//                    Chunks are merged by atomicMin on (ordered(key) << 32 | index): the minimum key, the lowest index among equals,
//                    whatever the order of arrival -- hence the same bits on every call.
//   The reverse direction of a mutual match is K21 launched again with the two sides exchanged: dot(i, j) is the same number either way
//   (the products commute, the order of b does not change), and the norm added is then qq.
//   K22 match_finish: one lane per query: the mutual filter and the match's distance in fp64.
// No scratch, no floating-point atomics.  Registers and LDS per instantiation: DESIGN.md, K20-K22.
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace mislam {

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

__global__ __launch_bounds__(256) void match_norms_kernel(const float* __restrict__ feat, int rows, int dim, float* __restrict__ norm, int* bad)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= rows) return;
    const float* r = feat + (size_t)i * (size_t)dim;
    float c = 0.f;
    bool ok = true;
    for (int b = 0; b < dim; b++) {
        const float v = r[b];
        ok = ok && (__builtin_fabsf(v) <= MATCH_MAX_ABS);            // false for a NaN
        c = __builtin_fmaf(v, v, c);
    }
    norm[i] = c;
    if (!ok) atomicMin(bad, i);
}

// a float as an unsigned that orders the same way (the keys are negative wherever 2 q.t > |t|^2)
__device__ __forceinline__ unsigned int match_ordered(float h)
{
    const unsigned int u = __float_as_uint(h);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// KS: k-steps of two components; the rows are zero-padded to 2 KS components in registers and in the LDS, which changes no bit of the chain
template <int KS>
__global__ __launch_bounds__(MATCH_BLOCK) void match_mfma_kernel(const MatchArgs a)
{
    constexpr int STRIDE = 2 * KS + 1;                               // odd: the 32 rows a half-wave reads fall into 32 different banks
    __shared__ float tile[MATCH_TILE * STRIDE];
    __shared__ float tnorm[MATCH_TILE];

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = lane & 31, half = lane >> 5;
    const int q = blockIdx.x * MATCH_TILE + wave * 32 + col;         // this lane's query (both halves of the wave hold the same 32)
    const int dim = a.dim;

    float qv[KS];                                                    // B operand: component 2 s + half of the lane's query
#pragma unroll
    for (int s = 0; s < KS; s++) {
        const int b = 2 * s + half;
        qv[s] = (q < a.n && b < dim) ? a.query[(size_t)q * (size_t)dim + b] : 0.f;
    }
    for (int e = threadIdx.x; e < MATCH_TILE * STRIDE; e += MATCH_BLOCK) tile[e] = 0.f;    // the padding columns stay zero from here on

    const int t_begin = blockIdx.y * a.chunk_len;
    const int t_end = min(a.m, t_begin + a.chunk_len);
    float best = __builtin_inff();                                   // every real key is finite (|component| <= 1e15)
    int best_j = 0x7fffffff;

    for (int t0 = t_begin; t0 < t_end; t0 += MATCH_TILE) {
        __syncthreads();                                             // the previous tile has been read (first trip: the zeros are in)
        const int rows = min(MATCH_TILE, t_end - t0);
        const float* src = a.target + (size_t)t0 * (size_t)dim;     // rows * dim consecutive floats
        for (int e = threadIdx.x; e < MATCH_TILE * dim; e += MATCH_BLOCK) {
            const int row = e / dim, b = e - row * dim;
            tile[row * STRIDE + b] = row < rows ? src[e] : 0.f;
        }
        if (threadIdx.x < MATCH_TILE) tnorm[threadIdx.x] = (int)threadIdx.x < rows ? a.target_norm[t0 + threadIdx.x] : __builtin_inff();
        __syncthreads();

        for (int sub = 0; sub < MATCH_TILE / 32; sub++) {
            if (sub * 32 >= rows) break;                             // wave-uniform
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; r++) acc[r] = 0.f;
            const float* arow = tile + (sub * 32 + col) * STRIDE + half;        // A operand: component 2 s + half of target sub * 32 + col
#pragma unroll
            for (int s = 0; s < KS; s++) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(arow[2 * s], qv[s], acc, 0, 0, 0);
            // acc[r] = dot(query col, target sub * 32 + row(r)), row(r) = (r & 3) + 8 (r >> 2) + 4 half: ascending in r
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int jl = sub * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                const float h = __builtin_fmaf(-2.0f, acc[r], tnorm[jl]);       // +inf beyond the chunk: never below best
                if (h < best) { best = h; best_j = t0 + jl; }
            }
        }
    }
    // the other half of the wave looked at the other targets of the same query
    const float oh = __shfl_xor(best, 32);
    const int oj = __shfl_xor(best_j, 32);
    if (oh < best || (oh == best && oj < best_j)) { best = oh; best_j = oj; }
    if (half == 0 && q < a.n && best_j != 0x7fffffff)
        atomicMin(&a.keys[q], ((unsigned long long)match_ordered(best) << 32) | (unsigned int)best_j);
}

__global__ __launch_bounds__(256) void match_finish_kernel(const MatchFinishArgs a)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    int j = (int)(unsigned int)(a.keys[i] & 0xffffffffull);
    if (j < 0 || j >= a.m) j = -1;                                   // (every query has met a target: does not happen)
    else if (a.rev_keys && (int)(unsigned int)(a.rev_keys[j] & 0xffffffffull) != i) j = -1;
    a.idx[i] = j;
    if (!a.d2) return;
    float out = __builtin_inff();
    if (j >= 0) {
        const float* qr = a.query + (size_t)i * (size_t)a.dim;
        const float* tr = a.target + (size_t)j * (size_t)a.dim;
        double s = 0.0;
        for (int b = 0; b < a.dim; b++) {
            const double d = (double)qr[b] - (double)tr[b];
            s = s + d * d;                                           // two roundings (the file is built with -ffp-contract=off)
        }
        out = (float)s;
    }
    a.d2[i] = out;
}

}  // namespace

hipError_t match_norms(const float* feat, int rows, int dim, float* norm, int* bad, hipStream_t s)
{
    if (rows < 1 || dim < 1 || dim > MATCH_MAX_DIM) return hipErrorInvalidValue;
    hipLaunchKernelGGL(match_norms_kernel, dim3((rows + 255) / 256), dim3(256), 0, s, feat, rows, dim, norm, bad);
    return hipGetLastError();
}

int match_chunk_len(int n, int m, int cu_count)
{
    const long long blocks = ((long long)n + MATCH_TILE - 1) / MATCH_TILE, tiles = ((long long)m + MATCH_TILE - 1) / MATCH_TILE;
    long long chunks = (2LL * cu_count + blocks - 1) / blocks;       // two workgroups per CU where the queries alone do not give them
    if (chunks < 1) chunks = 1;
    if (chunks > tiles) chunks = tiles;
    if (chunks > 65535) chunks = 65535;                              // grid.y
    return (int)((tiles + chunks - 1) / chunks) * MATCH_TILE;
}

hipError_t match_search(const MatchArgs& a, hipStream_t s)
{
    if (a.n < 1 || a.m < 1 || a.dim < 1 || a.dim > MATCH_MAX_DIM || a.chunk_len < MATCH_TILE || a.chunk_len % MATCH_TILE != 0) return hipErrorInvalidValue;
    const long long chunks = ((long long)a.m + a.chunk_len - 1) / a.chunk_len;
    if (chunks > 65535) return hipErrorInvalidValue;
    const dim3 grid((a.n + MATCH_TILE - 1) / MATCH_TILE, (unsigned int)chunks);
    if (a.dim <= 16) hipLaunchKernelGGL(match_mfma_kernel<8>, grid, dim3(MATCH_BLOCK), 0, s, a);
    else if (a.dim <= 34) hipLaunchKernelGGL(match_mfma_kernel<17>, grid, dim3(MATCH_BLOCK), 0, s, a);
    else hipLaunchKernelGGL(match_mfma_kernel<32>, grid, dim3(MATCH_BLOCK), 0, s, a);
    return hipGetLastError();
}

hipError_t match_finish(const MatchFinishArgs& a, hipStream_t s)
{
    if (a.n < 1 || a.dim < 1 || a.dim > MATCH_MAX_DIM) return hipErrorInvalidValue;
    hipLaunchKernelGGL(match_finish_kernel, dim3((a.n + 255) / 256), dim3(256), 0, s, a);
    return hipGetLastError();
}

// loads this translation unit's code object at mi_ctx_preload (kernels.h)
__global__ void preload_match_kernels_kernel() {}
hipError_t preload_match_kernels()
{
    hipFuncAttributes attr;
    return hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(preload_match_kernels_kernel));
}

}  // namespace mislam
