// K-batch CPD -- many small exact-P registrations in one launch: ONE WORKGROUP PER PROBLEM, the EM iterations inside the kernel.
//
// One EM iteration of mi_cpd_register is six launches (cpd_kernels.hip: denominators, post, contraction, post, solve, transform) of which
// none fills more than a fraction of the device for a cloud of a thousand points: the registration is bound by launch boundaries and host
// checks.  Inside one workgroup those boundaries are __syncthreads(), and the device carries as many registrations side by side as it
// has room for workgroups.
//
//   cpd_batch_init_kernel      per problem: the eight sums of the two clouds in the rows of cpd_init_sums_kernel, reduce_partials, the
//                              state at sigma^2_0 (cpd_init_state_body).
//   cpd_batch_iterate_kernel   per problem, up to `iters` EM iterations: the moving cloud's current positions into LDS, denominators
//                              (lanes own fixed points), Pt1 / xw4 and the x-sums rows, the fixed cloud into LDS, contraction on the
//                              matrix pipe (a wave owns 64 moving points), P1 / PX and the k-sums rows, reduce + solve on one lane.
//
// The bits are those of mi_cpd_register.  Every fp32 sum is added in the single path's order, which the problem's chunking fixes
// (CpdBatchProblem: plan_chunks of the single path, evaluated by the host for these sizes):
//   a fixed point's denominator   per k-chunk a running sum from 0 over the moving points in index order (cpd_denominator_kernel), the chunk
//                                 sums added per quarter of the chunks in chunk order, the quarters ((s0 + s1) + s2) + s3 (cpd_post_den_kernel);
//   a moving point's P1 / PX      per x-chunk the v_mfma_f32_4x4x1 chain from 0 over the fixed points in index order (cpd_contract_mfma_kernel),
//                                 the chunk sums per quarter, the quarters in the same order (cpd_post_contract_kernel);
//   the M-step's fp64 moments     one row per 64 points, produced by the 256 threads of a post kernel's workgroup -- a quad of lanes per
//                                 point, the quad's first lane holding the terms -- and block_sum_store: here the workgroup takes the rows one
//                                 after the other in that very layout; then reduce_partials and cpd_solve_body as cpd_solve_kernel runs them.
// The single path's partial arrays (den_part, p1_part, px_part) do not exist here: a lane keeps the running chunk sum, the quarter's sum
// and the total in registers.
//
// Bounded launches: a launch carries at most `iters` iterations per problem and ends; between launches a problem is its CpdState block
// and its two clouds in global memory -- the current moving cloud is s R b + t, recomputed from the state wherever it is needed exactly
// as cpd_transform_kernel computes it (before the first M-step it is b itself, as the single path's copy).  Every workgroup whose problem
// is still running adds one to a counter the host reads: zero ends the call.  No cooperative launch, no grid barrier, no flag of another
// workgroup is ever waited for, no float atomics.
#include <hip/hip_runtime.h>

#include "cpd_kernels.h"
#include "cpd_math.hpp"
#include "reduce.hpp"

namespace mislam {

constexpr int CB_THREADS = 256;                          // the workgroup of every single-path kernel whose sums are replayed here
constexpr int CB_WAVES = CB_THREADS / 64;
constexpr int CB_MAX_ROWS = CPD_BATCH_MAX_POINTS / 64;   // rows of M-step partial sums per cloud (cpd_sum_blocks)
static_assert(CPD_BATCH_MAX_POINTS / 256 <= CB_MAX_ROWS, "the init sums' rows fit the x-rows buffer");
static_assert(CPD_BATCH_MAX_POINTS / 64 <= ICP_MAX_PARTIAL_BLOCKS, "one row per 64 points: the post kernels make a single trip");

// The workgroup's LDS, carved from the dynamic region (every offset a multiple of 16 bytes).  P = points rounded up to 64.
struct CbLayout {
    size_t sw, xrows, krows, red, st, cbuf, sx, sy, sz, spt1, total;
    __host__ __device__ explicit CbLayout(int max_points)
    {
        const size_t P = ((size_t)max_points + 63) / 64 * 64;
        size_t o = 0;
        sw = o; o += 16 * P;                                              // xw4 records of the fixed cloud
        xrows = o; o += sizeof(double) * CB_MAX_ROWS * CPD_XSUMS;
        krows = o; o += sizeof(double) * CB_MAX_ROWS * CPD_KSUMS;
        red = o; o += sizeof(double) * 256;                               // reduce_partials' scratch
        st = o; o += (sizeof(CpdState) + 15) / 16 * 16;
        cbuf = o; o += sizeof(float) * CB_WAVES * 256;                    // a round's P1 / PX: per wave [4][64]
        sx = o; o += 4 * P; sy = o; o += 4 * P; sz = o; o += 4 * P;       // the cloud that is streamed: moving (denominators), fixed (contraction)
        spt1 = o; o += 4 * P;
        total = o;
    }
};
size_t cpd_batch_lds_bytes(int max_points) { return CbLayout(max_points).total; }

static __device__ __forceinline__ int cb_init_rows(int m, int n)        // icp_reduce_blocks(max(m, n))
{
    int b = ((m > n ? m : n) + 255) / 256;
    if (b > ICP_MAX_PARTIAL_BLOCKS) b = ICP_MAX_PARTIAL_BLOCKS;
    return b < 1 ? 1 : b;
}

// ---------------------------------------------------------------------------------------------------------------
// the state at sigma^2_0
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CB_THREADS) void cpd_batch_init_kernel(CpdBatchArgs a)
{
    __shared__ double rows[(CPD_BATCH_MAX_POINTS / 256) * CPD_INIT_SUMS];
    __shared__ double lds[256];
    const CpdBatchProblem p = a.problems[blockIdx.x];
    const float* __restrict__ after = a.after + 3 * (size_t)p.a_off;
    const float* __restrict__ before = a.before + 3 * (size_t)p.b_off;
    const int nb = cb_init_rows(p.m, p.n);
    for (int vb = 0; vb < nb; vb++) {                    // workgroup vb of cpd_init_sums_kernel
        double acc[CPD_INIT_SUMS] = {0};
        for (int i = vb * 256 + (int)threadIdx.x; i < p.n; i += nb * 256) {
            const double x = after[3 * (size_t)i], y = after[3 * (size_t)i + 1], z = after[3 * (size_t)i + 2];
            acc[0] += x; acc[1] += y; acc[2] += z; acc[3] += x * x + y * y + z * z;
        }
        for (int i = vb * 256 + (int)threadIdx.x; i < p.m; i += nb * 256) {
            const double x = before[3 * (size_t)i], y = before[3 * (size_t)i + 1], z = before[3 * (size_t)i + 2];
            acc[4] += x; acc[5] += y; acc[6] += z; acc[7] += x * x + y * y + z * z;
        }
        block_sum_store<CPD_INIT_SUMS>(acc, rows + vb * CPD_INIT_SUMS);
        __syncthreads();                                 // the row is written; block_sum_store's scratch is free again
    }
    double s[CPD_INIT_SUMS];
    reduce_partials<CPD_INIT_SUMS>(rows, nb, s, lds);
    if (threadIdx.x != 0) return;
    CpdRules rules = a.rules;
    rules.m = p.m; rules.n = p.n;
    cpd_init_state_body(a.states + blockIdx.x, s, rules, a.sigma2_override, 0);
}

// ---------------------------------------------------------------------------------------------------------------
// the loop
// ---------------------------------------------------------------------------------------------------------------
// K7a + the per-point part of cpd_post_den_kernel: a lane owns R fixed points per pass, the moving cloud streams out of LDS.
template <int R>
__device__ __forceinline__ void cb_denominators(const CpdBatchProblem& p, const float* __restrict__ after, const float* sx, const float* sy,
                                                const float* sz, float mult, float c, float4* sw, float* spt1)
{
    for (int base = 0; base < p.n; base += CB_THREADS * R) {
        const int x0 = base + (int)threadIdx.x;
        float ax[R], ay[R], az[R], tot[R];
#pragma unroll
        for (int r = 0; r < R; r++) {
            const int i = min(x0 + r * CB_THREADS, p.n - 1);
            ax[r] = after[3 * (size_t)i]; ay[r] = after[3 * (size_t)i + 1]; az[r] = after[3 * (size_t)i + 2];
            tot[r] = 0.f;
        }
        for (int q = 0; q < 4; q++) {                    // the quad lane `part` of cpd_post_den_kernel: its quarter of the chunks, in chunk order
            const int ch_lo = (int)((long long)p.k_chunks * q / 4), ch_hi = (int)((long long)p.k_chunks * (q + 1) / 4);
            float sq[R];
#pragma unroll
            for (int r = 0; r < R; r++) sq[r] = 0.f;
            for (int ch = ch_lo; ch < ch_hi; ch++) {
                const int k_begin = ch * p.k_chunk_len;
                const int k_end = min(k_begin + p.k_chunk_len, p.m);
                float cs[R];
#pragma unroll
                for (int r = 0; r < R; r++) cs[r] = 0.f;
                int k = k_begin;
                for (; k + CPD_T <= k_end; k += CPD_T) {
#pragma unroll
                    for (int u = 0; u < CPD_T; u++) {
                        const float yx = sx[k + u], yy = sy[k + u], yz = sz[k + u];
#pragma unroll
                        for (int r = 0; r < R; r++) cs[r] += affinity<false>(mult * sq_dist(ax[r], ay[r], az[r], yx, yy, yz), 0.f);
                    }
                }
                for (; k < k_end; k++) {
                    const float yx = sx[k], yy = sy[k], yz = sz[k];
#pragma unroll
                    for (int r = 0; r < R; r++) cs[r] += affinity<false>(mult * sq_dist(ax[r], ay[r], az[r], yx, yy, yz), 0.f);
                }
#pragma unroll
                for (int r = 0; r < R; r++) sq[r] += cs[r];
            }
#pragma unroll
            for (int r = 0; r < R; r++) tot[r] = q == 0 ? sq[r] : tot[r] + sq[r];      // ((s0 + s1) + s2) + s3
        }
#pragma unroll
        for (int r = 0; r < R; r++) {
            const int i = x0 + r * CB_THREADS;
            if (i < p.n) {
                float den = tot[r];
                den += c;
                const float w = 1.0f / den;
                const float pt1 = 1.0f - c / den;
                spt1[i] = pt1;
                sw[i] = make_float4(ax[r] * w, ay[r] * w, az[r] * w, w);
            }
        }
    }
}

// K7b + the per-point part of cpd_post_contract_kernel for the 64 moving points of one wave: lane l holds, in the D layout of the
// 4x4x1 form, component j = l & 3 (0..2: PX, 3: P1) of the points 4 (l >> 2) + i, i = 0..3.
__device__ __forceinline__ f32x4 cb_contract_group(const CpdBatchProblem& p, float yx, float yy, float yz, const float* sx, const float* sy,
                                                   const float* sz, const float* wrec, float mult, int lane)
{
    const int j = lane & 3;
    f32x4 tot = {0.f, 0.f, 0.f, 0.f};
    for (int q = 0; q < 4; q++) {
        const int ch_lo = (int)((long long)p.x_chunks * q / 4), ch_hi = (int)((long long)p.x_chunks * (q + 1) / 4);
        f32x4 sq = {0.f, 0.f, 0.f, 0.f};
        for (int ch = ch_lo; ch < ch_hi; ch++) {
            const int x_begin = ch * p.x_chunk_len;
            const int x_end = min(x_begin + p.x_chunk_len, p.n);
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            // two fixed points at a time as packed operations (bit for bit two single affinities); the matrix instructions stay in x order
            auto pair = [&](int xx) {
                const cpd_f32x2 pp = affinity2<false>(mult, (cpd_f32x2){sx[xx], sx[xx + 1]}, (cpd_f32x2){sy[xx], sy[xx + 1]}, (cpd_f32x2){sz[xx], sz[xx + 1]},
                                                      yx, yy, yz, 0.f);
                acc = __builtin_amdgcn_mfma_f32_4x4x1f32(pp.x, wrec[4 * xx + j], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_4x4x1f32(pp.y, wrec[4 * (xx + 1) + j], acc, 0, 0, 0);
            };
            int x = x_begin;
            for (; x + CPD_T <= x_end; x += CPD_T) {
#pragma unroll
                for (int u = 0; u < CPD_T; u += 2) pair(x + u);
            }
            for (; x + 2 <= x_end; x += 2) pair(x);
            if (x < x_end) {
                const float pr = affinity<false>(mult * sq_dist(sx[x], sy[x], sz[x], yx, yy, yz), 0.f);
                acc = __builtin_amdgcn_mfma_f32_4x4x1f32(pr, wrec[4 * x + j], acc, 0, 0, 0);
            }
            sq = sq + acc;
        }
        tot = q == 0 ? sq : tot + sq;
    }
    return tot;
}

// The one-lane solve as a real call: inlined, the 3 x 3 SVD's registers would come on top of the E-step loops'.
// (the moments travel through the state block in LDS, where cpd_solve_body leaves them anyway: handed over as references to lane 0's
// registers they become a 336-byte frame per lane instead of 128)
__device__ __attribute__((noinline)) void cb_solve(CpdState* st, CpdRules rules)
{
    double xs[CPD_XSUMS], ks[CPD_KSUMS];
    for (int i = 0; i < CPD_XSUMS; i++) xs[i] = st->xs[i];
    for (int i = 0; i < CPD_KSUMS; i++) ks[i] = st->ks[i];
    cpd_solve_body(st, xs, ks, rules, 1);
}

__global__ __launch_bounds__(CB_THREADS) void cpd_batch_iterate_kernel(CpdBatchArgs a)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    CpdState* __restrict__ gst = a.states + blockIdx.x;
    if (gst->done != 0) return;                          // (uniform: the state is only written by this workgroup, in the launch before)
    const CbLayout L(a.max_points);
    float4* sw = reinterpret_cast<float4*>(smem + L.sw);
    double* xrows = reinterpret_cast<double*>(smem + L.xrows);
    double* krows = reinterpret_cast<double*>(smem + L.krows);
    double* red = reinterpret_cast<double*>(smem + L.red);
    CpdState* st = reinterpret_cast<CpdState*>(smem + L.st);
    float* cbuf = reinterpret_cast<float*>(smem + L.cbuf);
    float* sx = reinterpret_cast<float*>(smem + L.sx);
    float* sy = reinterpret_cast<float*>(smem + L.sy);
    float* sz = reinterpret_cast<float*>(smem + L.sz);
    float* spt1 = reinterpret_cast<float*>(smem + L.spt1);

    const CpdBatchProblem p = a.problems[blockIdx.x];
    const float* __restrict__ after = a.after + 3 * (size_t)p.a_off;
    const float* __restrict__ before = a.before + 3 * (size_t)p.b_off;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr int WORDS = (int)(sizeof(CpdState) / sizeof(int));
    static_assert(sizeof(CpdState) % sizeof(int) == 0, "the state block is copied word by word");
    for (int i = tid; i < WORDS; i += CB_THREADS) reinterpret_cast<int*>(st)[i] = reinterpret_cast<const int*>(gst)[i];
    __syncthreads();
    CpdRules rules = a.rules;
    rules.m = p.m; rules.n = p.n;
    const int nxb = (p.n + 63) / 64, nkb = (p.m + 63) / 64;        // cpd_sum_blocks: rows of M-step partial sums

    for (int it = 0; it < a.iters; it++) {
        const bool moved = st->iterations > 0;           // the first E-step reads the moving cloud as it was given (transformedCloud = cloudBefore)
        const float mult = -0.5f / st->sigma2;           // coherentpointdrift.cpp:176
        const float c = st->constant;
        // ---- the moving cloud's current positions: the stream of the denominators
        for (int k = tid; k < p.m; k += CB_THREADS) {
            float x = before[3 * (size_t)k], y = before[3 * (size_t)k + 1], z = before[3 * (size_t)k + 2];
            if (moved) cpd_transform_point(st, x, y, z, &x, &y, &z);
            sx[k] = x; sy[k] = y; sz[k] = z;
        }
        __syncthreads();
        // ---- K7a: denominators, Pt1, xw4
        if (p.n <= CB_THREADS) cb_denominators<1>(p, after, sx, sy, sz, mult, c, sw, spt1);
        else if (p.n <= 2 * CB_THREADS) cb_denominators<2>(p, after, sx, sy, sz, mult, c, sw, spt1);
        else cb_denominators<4>(p, after, sx, sy, sz, mult, c, sw, spt1);
        __syncthreads();
        // ---- the x-sums, row by row in the thread layout of cpd_post_den_kernel; the fixed cloud replaces the moving one as the stream
        for (int vb = 0; vb < nxb; vb++) {
            double acc[CPD_XSUMS] = {0};
            const int i = vb * 64 + (tid >> 2);
            if (i < p.n && (tid & 3) == 0) {
                const float w = sw[i].w, pt1 = spt1[i];
                const float x = after[3 * (size_t)i], y = after[3 * (size_t)i + 1], z = after[3 * (size_t)i + 2];
                acc[0] += (double)logf(1.0f / w);                           // error -= log(denominator), :215
                acc[1] += (double)x * pt1; acc[2] += (double)y * pt1; acc[3] += (double)z * pt1;
                acc[4] += (double)(x * x) * pt1 + (double)(y * y) * pt1 + (double)(z * z) * pt1;     // :257
            }
            block_sum_store<CPD_XSUMS>(acc, xrows + vb * CPD_XSUMS);
            __syncthreads();
        }
        for (int x = tid; x < p.n; x += CB_THREADS) { sx[x] = after[3 * (size_t)x]; sy[x] = after[3 * (size_t)x + 1]; sz[x] = after[3 * (size_t)x + 2]; }
        __syncthreads();
        // ---- K7b: contraction, a round of CB_WAVES groups of 64 moving points at a time; then the round's k-sums rows
        for (int g0 = 0; g0 < nkb; g0 += CB_WAVES) {
            const int g = g0 + wave;
            if (g < nkb) {                               // (wave-uniform: every lane of the wave reaches the matrix instructions)
                const int kc = min(g * 64 + lane, p.m - 1);
                float yx = before[3 * (size_t)kc], yy = before[3 * (size_t)kc + 1], yz = before[3 * (size_t)kc + 2];
                if (moved) cpd_transform_point(st, yx, yy, yz, &yx, &yy, &yz);
                const f32x4 tot = cb_contract_group(p, yx, yy, yz, sx, sy, sz, reinterpret_cast<const float*>(sw), mult, lane);
                float* out = cbuf + wave * 256 + (lane & 3) * 64 + 4 * (lane >> 2);
#pragma unroll
                for (int i = 0; i < 4; i++) out[i] = tot[i];
            }
            __syncthreads();
            const int g1 = min(g0 + CB_WAVES, nkb);
            for (int vb = g0; vb < g1; vb++) {           // the thread layout of cpd_post_contract_kernel
                double acc[CPD_KSUMS] = {0};
                const int kl = tid >> 2, k = vb * 64 + kl;
                if (k < p.m && (tid & 3) == 0) {
                    const float* rec = cbuf + (vb - g0) * 256;
                    const float p1 = rec[3 * 64 + kl];
                    const float px[3] = {rec[kl], rec[64 + kl], rec[2 * 64 + kl]};
                    const float b[3] = {before[3 * (size_t)k], before[3 * (size_t)k + 1], before[3 * (size_t)k + 2]};
                    acc[0] += (double)p1;
                    for (int r = 0; r < 3; r++) {
                        acc[1 + r] += (double)b[r] * p1;
                        for (int cc = 0; cc < 3; cc++) acc[4 + 3 * r + cc] += (double)b[r] * px[cc];
                        acc[13] += (double)(b[r] * b[r]) * p1;                                            // :259
                    }
                }
                block_sum_store<CPD_KSUMS>(acc, krows + vb * CPD_KSUMS);
                __syncthreads();
            }
        }
        // ---- K8: the rows reduced as cpd_solve_kernel reduces them, the solve and the stop rule on one lane
        double xs[CPD_XSUMS], ks[CPD_KSUMS];
        reduce_partials<CPD_XSUMS>(xrows, nxb, xs, red);
        reduce_partials<CPD_KSUMS>(krows, nkb, ks, red);
        if (tid == 0) {
            for (int i = 0; i < CPD_XSUMS; i++) st->xs[i] = xs[i];
            for (int i = 0; i < CPD_KSUMS; i++) st->ks[i] = ks[i];
            cb_solve(st, rules);
        }
        __syncthreads();
        if (st->done != 0) break;
    }
    __syncthreads();
    for (int i = tid; i < WORDS; i += CB_THREADS) reinterpret_cast<int*>(gst)[i] = reinterpret_cast<const int*>(st)[i];
    if (tid == 0 && st->done == 0) atomicAdd(a.running, 1);
}

// ---------------------------------------------------------------------------------------------------------------
// host-side launchers
// ---------------------------------------------------------------------------------------------------------------
hipError_t cpd_batch_init(const CpdBatchArgs& a, hipStream_t s)
{
    if (a.n_problems <= 0) return hipSuccess;
    hipLaunchKernelGGL(cpd_batch_init_kernel, dim3(a.n_problems), dim3(CB_THREADS), 0, s, a);
    return hipGetLastError();
}

hipError_t cpd_batch_iterate(const CpdBatchArgs& a, hipStream_t s)
{
    if (a.n_problems <= 0 || a.iters <= 0 || a.max_points < 1 || a.max_points > CPD_BATCH_MAX_POINTS) return hipErrorInvalidValue;
    const size_t lds = cpd_batch_lds_bytes(a.max_points);
    if (lds > 48 * 1024) {                               // beyond the default limit of dynamically sized LDS the kernel has to be told
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(cpd_batch_iterate_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(cpd_batch_iterate_kernel, dim3(a.n_problems), dim3(CB_THREADS), lds, s, a);
    return hipGetLastError();
}

__global__ void preload_cpd_batch_kernel() {}
hipError_t preload_cpd_batch()
{
    hipFuncAttributes attr;
    return hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(preload_cpd_batch_kernel));
}

}  // namespace mislam
