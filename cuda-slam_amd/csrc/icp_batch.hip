// K-batch -- many small ICP registrations in one launch: ONE WORKGROUP PER PROBLEM, the iterations inside the kernel.
//
// A registration of a few thousand points is four launches per iteration of which none fills more than a fraction of a CU
// (icp_kernels.hip): it is bound by launch boundaries and host checks.  Spread over the grid, a whole-loop
// kernel would need a grid barrier per phase; with one problem per workgroup __syncthreads() is the only synchronisation an
// iteration needs, and the device carries as many registrations side by side as it has room for workgroups.
//
//   icp_batch_prepare_kernel   per problem: bounding box of the moving cloud, the 30-bit curve codes in that box
//                              (curve_code.hpp, as morton_order forms them), a stable ordering by code (bitonic network on
//                              the unique keys code << 12 | index = what the stable radix sort yields), the sorted cloud
//                              as SoA, the state block at identity.
//   icp_batch_iterate_kernel   per problem, up to `iters` loop bodies of basicicp.cpp:32-57 / icpcuda.cu:31-54: every-pair
//                              search (fixed points streamed through LDS in tiles, strict '<', ascending index), one row of
//                              moments per 64 sorted points (row_store_pair_moments), the rows added up in the strip order
//                              of icp_rows_reduce_kernel / icp_reduce_solve_kernel, reduce_rows_wave, apply_solve,
//                              transform in glm order, row_store_error, the same reduce, finalize_iteration.
//
// The bits are those of mi_icp_register: every sum is produced by the producer functions of icp_rows.hpp and added in the order
// the stand-alone kernels add it, the solve and the stop rules are the device functions of icp_solve.hpp.  The single call defers an
// iteration's stop rule into the next iteration's solve launch to save a launch; inside one workgroup nothing is saved by that, so
// here the rule is evaluated right behind the error sums -- the same calls with the same arguments in the same order, one search
// earlier.
//
// Bounded launches: a launch carries at most `iters` iterations per problem and ends; what a problem needs to go on -- its state
// block; the current cloud is R * sorted + t, recomputed on entry exactly as the iteration that produced it computed it -- lives in
// global memory.  Every workgroup whose problem is still running adds one to a counter the host reads: zero ends the call.  No
// cooperative launch, no grid barrier, no flag of another workgroup is ever waited for, no float atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "curve_code.hpp"
#include "icp_rows.hpp"
#include "icp_solve.hpp"
#include "kernels.h"

namespace mislam {

constexpr int BATCH_THREADS = 512;                       // 8 waves
constexpr int BATCH_WAVES = BATCH_THREADS / 64;
constexpr int BATCH_TILE = 2048;                         // fixed points per LDS tile (32 KiB as float4)
constexpr int BATCH_MAX_ROWS = ICP_BATCH_MAX_MOVING / ICP_ROW_POINTS;   // 64 rows of 64 points
static_assert(BATCH_MAX_ROWS <= BATCH_WAVES * 8, "a lane carries at most 8 moving points");
static_assert(BATCH_MAX_ROWS <= 2 * 32, "the rows of a problem reduce to at most two strips-slices of <= 32 rows (icp_reduced_count)");
static_assert(ICP_BATCH_MAX_MOVING <= 4096, "the sort key keeps the index in 12 bits");

// ---------------------------------------------------------------------------------------------------------------
// load stage
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BATCH_THREADS) void icp_batch_prepare_kernel(IcpBatchArgs a)
{
    __shared__ unsigned long long skey[ICP_BATCH_MAX_MOVING];
    __shared__ float sbox[6][BATCH_THREADS];
    __shared__ float bbox[6];
    const IcpBatchProblem p = a.problems[blockIdx.x];
    const float* __restrict__ src = a.before + 3 * (size_t)p.b_off;
    const int tid = threadIdx.x;
    // the box: min / max do not depend on the order they are taken in
    float lo[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()};
    float hi[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
    for (int j = tid; j < p.n; j += BATCH_THREADS)
        for (int c = 0; c < 3; c++) { const float v = src[3 * (size_t)j + c]; lo[c] = fminf(lo[c], v); hi[c] = fmaxf(hi[c], v); }
    for (int c = 0; c < 3; c++) { sbox[c][tid] = lo[c]; sbox[3 + c][tid] = hi[c]; }
    __syncthreads();
    for (int w = BATCH_THREADS / 2; w > 0; w >>= 1) {
        if (tid < w)
            for (int c = 0; c < 3; c++) {
                sbox[c][tid] = fminf(sbox[c][tid], sbox[c][tid + w]);
                sbox[3 + c][tid] = fmaxf(sbox[3 + c][tid], sbox[3 + c][tid + w]);
            }
        __syncthreads();
    }
    if (tid < 6) bbox[tid] = sbox[tid][0];
    __syncthreads();
    int len = 1;
    while (len < p.n) len <<= 1;
    for (int j = tid; j < len; j += BATCH_THREADS) {
        unsigned long long key = ~0ull;                  // padding sorts behind every point
        if (j < p.n) {
            const float q[3] = {src[3 * (size_t)j], src[3 * (size_t)j + 1], src[3 * (size_t)j + 2]};
            key = ((unsigned long long)curve_code30(q, bbox) << 12) | (unsigned int)j;
        }
        skey[j] = key;
    }
    __syncthreads();
    // bitonic network, ascending.  The keys are unique (the index is part of them), so the result is THE sorted sequence: points in code
    // order, equal codes in the caller's order -- what the stable radix sort on the codes yields.
    for (int k = 2; k <= len; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < len; i += BATCH_THREADS) {
                const int l = i ^ j;
                if (l > i) {
                    const unsigned long long x = skey[i], y = skey[l];
                    const bool up = (i & k) == 0;
                    if ((x > y) == up) { skey[i] = y; skey[l] = x; }
                }
            }
            __syncthreads();
        }
    for (int s = tid; s < p.n; s += BATCH_THREADS) {
        const int j = (int)(skey[s] & 0xfffu);
        a.sx[p.s_off + s] = src[3 * (size_t)j];
        a.sy[p.s_off + s] = src[3 * (size_t)j + 1];
        a.sz[p.s_off + s] = src[3 * (size_t)j + 2];
    }
    if (tid == 0) {                                      // state_identity + the reset rule of mi_icp_reset
        IcpState* st = a.states + blockIdx.x;
        int* w = reinterpret_cast<int*>(st);
        for (int i = 0; i < (int)(sizeof(IcpState) / sizeof(int)); i++) w[i] = 0;
        st->R[0] = st->R[4] = st->R[8] = 1.f;
        st->prevR[0] = st->prevR[4] = st->prevR[8] = 1.f;
        st->error = 1e5f;
        st->prev_error = 3.402823466e38f;
        if (a.rules.max_iterations == 0) { st->done = 1; st->stop_reason = MI_STOP_MAX_ITERATIONS_; }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// the loop
// ---------------------------------------------------------------------------------------------------------------
template <bool FMA>
__device__ __forceinline__ float batch_dist2(float tx, float ty, float tz, float sx, float sy, float sz)
{
    const float dx = tx - sx, dy = ty - sy, dz = tz - sz;      // target - source, as K1 and K4+K5 form it
    if (FMA)
        return __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
    else
        return (dx * dx + dy * dy) + dz * dz;
}

// What the workgroup shares.  One struct, so that the kernel body and its helpers name the same arrays.
struct BatchShared {
    float4 tile[BATCH_TILE];
    double rows[BATCH_MAX_ROWS * ICP_ROW];
    double part[2 * ICP_ROW];
    double sums[ICP_ROW];
    unsigned long long merge[BATCH_WAVES * 64];
    IcpState st;
};

// rows [0, nrows) -> sums[0..18): the slices and strips of icp_rows_reduce_kernel as icp_reduce_solve_kernel replays them (a slice has
// at most 32 rows here, one per strip: 0.0 + row, the strips in order, the empty ones adding their 0.0), then the butterfly over
// the <= 2 reduced rows.  Every thread calls it; sums is valid on return.
__device__ __forceinline__ void batch_reduce_rows(BatchShared& sh, int nrows, int rows_per_block, int count)
{
    constexpr int SLICE = 32, STRIPS = 1024 / ICP_ROW;
    __syncthreads();
    for (int item = (int)threadIdx.x; item < count * ICP_ROW; item += BATCH_THREADS) {
        const int b = item / ICP_ROW, k = item - b * ICP_ROW;
        const int lo = b * rows_per_block;
        const int hi = lo + rows_per_block < nrows ? lo + rows_per_block : nrows;
        double tot = 0.0;                                // (0.0 + row 0, then + (0.0 + row j): the loads eight at a time, the additions one chain)
#pragma unroll
        for (int j0 = 0; j0 < SLICE; j0 += 8) {
            double val[8];
#pragma unroll
            for (int j = 0; j < 8; j++) val[j] = lo + j0 + j < hi ? sh.rows[(lo + j0 + j) * ICP_ROW + k] : 0.0;
#pragma unroll
            for (int j = 0; j < 8; j++) tot = tot + (0.0 + val[j]);
        }
        if (SLICE < STRIPS) tot = tot + 0.0;
        sh.part[item] = tot;
    }
    __syncthreads();
    reduce_rows_wave(sh.part, count, sh.sums);           // (every wave computes the same 18 sums and stores the same values)
}

// The one-lane parts of an iteration as real calls: inlined, their registers (the 3 x 3 SVD alone takes ~90) would come on top of the eight
// moving points a lane carries through the search in every one of the four instantiations below.
__device__ __attribute__((noinline)) void batch_solve(BatchShared* sh, int compose_mode, int svd_ieee)
{
    double mom[ICP_MOMENTS];
    for (int i = 0; i < ICP_MOMENTS; i++) { mom[i] = sh->sums[i]; sh->st.mom[i] = sh->sums[i]; }
    apply_solve(&sh->st, mom, compose_mode, 0, svd_ieee);
}
__device__ __attribute__((noinline)) void batch_finalize(BatchShared* sh, const IcpRules* rules)
{
    sh->st.err[0] = sh->sums[ICP_MOMENTS];
    sh->st.err[1] = sh->sums[ICP_MOMENTS + 1];
    finalize_iteration(&sh->st, sh->sums[ICP_MOMENTS], sh->sums[ICP_MOMENTS + 1], *rules);
}

// R moving points per lane.  P == 1: wave w owns rows w, w + 8, ...; P > 1 (at most four rows): P waves share a row, each scanning its
// part of every tile, the lanes' packed (d2, index) keys merged by minimum -- the key's order is strict '<' with the lowest index on ties.
template <int R, bool FMA>
__device__ __forceinline__ void batch_run(const IcpBatchArgs& a, const IcpBatchProblem& p, BatchShared& sh)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nrows = (p.n + ICP_ROW_POINTS - 1) / ICP_ROW_POINTS;
    int g = (nrows + 31) / 32;                           // icp_reduced_count / icp_reduce_solve
    if (g < 1) g = 1;
    const int per = (nrows + g - 1) / g;
    int parts = 1, slots = BATCH_WAVES;
    if (R == 1 && nrows <= 4) { slots = nrows <= 1 ? 1 : (nrows <= 2 ? 2 : 4); parts = BATCH_WAVES / slots; }
    const int part = wave / slots, row0 = wave % slots;
    const float* __restrict__ after = a.after + 3 * (size_t)p.a_off;
    const float* __restrict__ bx = a.sx + p.s_off;
    const float* __restrict__ by = a.sy + p.s_off;
    const float* __restrict__ bz = a.sz + p.s_off;
    IcpRules rules = a.rules;
    rules.m_total = p.m;

    int pt[R];
    bool valid[R], row_ok[R];
    float cx[R], cy[R], cz[R];
#pragma unroll
    for (int r = 0; r < R; r++) {
        const int row = row0 + r * BATCH_WAVES;
        const int i = row * ICP_ROW_POINTS + lane;
        row_ok[r] = row < nrows && part == 0;            // this wave writes the row's sums
        valid[r] = i < p.n;
        pt[r] = valid[r] ? i : p.n - 1;
        cx[r] = bx[pt[r]]; cy[r] = by[pt[r]]; cz[r] = bz[pt[r]];
    }
    if (sh.st.passes > 0) {                              // a later launch: the current cloud is the last applied transform of the sorted one
        float Rm[9], t[3];
#pragma unroll
        for (int i = 0; i < 9; i++) Rm[i] = sh.st.R[i];
#pragma unroll
        for (int i = 0; i < 3; i++) t[i] = sh.st.t[i];
#pragma unroll
        for (int r = 0; r < R; r++) {
            const float x = cx[r], y = cy[r], z = cz[r];
            cx[r] = ((Rm[0] * x + Rm[3] * y) + Rm[6] * z) + t[0];
            cy[r] = ((Rm[1] * x + Rm[4] * y) + Rm[7] * z) + t[1];
            cz[r] = ((Rm[2] * x + Rm[5] * y) + Rm[8] * z) + t[2];
        }
    }

    for (int it = 0; it < a.iters; it++) {
        // ---- K1: every pair
        float best[R];
        int bidx[R];
#pragma unroll
        for (int r = 0; r < R; r++) { best[r] = __builtin_inff(); bidx[r] = -1; }
        for (int t0 = 0; t0 < p.m; t0 += BATCH_TILE) {
            const int len = p.m - t0 < BATCH_TILE ? p.m - t0 : BATCH_TILE;
            __syncthreads();                             // the tile's previous readers are through
            for (int j = tid; j < len; j += BATCH_THREADS) {
                const float* q = after + 3 * (size_t)(t0 + j);
                sh.tile[j] = make_float4(q[0], q[1], q[2], 0.f);
            }
            __syncthreads();
            const int chunk = (len + parts - 1) / parts;
            const int jlo = part * chunk, jhi = jlo + chunk < len ? jlo + chunk : len;
#pragma unroll 4
            for (int j = jlo; j < jhi; j++) {
                const float4 q = sh.tile[j];
#pragma unroll
                for (int r = 0; r < R; r++) {
                    const float d = batch_dist2<FMA>(q.x, q.y, q.z, cx[r], cy[r], cz[r]);
                    if (d < best[r]) { best[r] = d; bidx[r] = t0 + j; }
                }
            }
        }
        unsigned int dbits[R];
#pragma unroll
        for (int r = 0; r < R; r++) dbits[r] = bidx[r] >= 0 ? __float_as_uint(best[r]) : 0xffffffffu;     // no candidate: KEY_INIT
        if (R == 1 && parts > 1) {
            sh.merge[wave * 64 + lane] = ((unsigned long long)dbits[0] << 32) | (unsigned int)bidx[0];
            __syncthreads();
            unsigned long long key = sh.merge[row0 * 64 + lane];
            for (int q = 1; q < parts; q++) {
                const unsigned long long other = sh.merge[(q * slots + row0) * 64 + lane];
                key = other < key ? other : key;
            }
            dbits[0] = (unsigned int)(key >> 32);
            bidx[0] = (int)(unsigned int)(key & 0xffffffffull);
        }
        // ---- K2: moments rows
#pragma unroll
        for (int r = 0; r < R; r++) {
            if (!row_ok[r]) continue;                    // (wave-uniform)
            const bool mine = bidx[r] >= 0 && bidx[r] < p.m;
            const bool kept = rules.filter_pairs ? (__uint_as_float(dbits[r]) < a.max_distance_squared) : true;
            const bool use = valid[r] && mine && kept;
            float ax = 0.f, ay = 0.f, az = 0.f;
            if (use) { const float* q = after + 3 * (size_t)bidx[r]; ax = q[0]; ay = q[1]; az = q[2]; }
            row_store_pair_moments(use, cx[r], cy[r], cz[r], ax, ay, az, sh.rows + (row0 + r * BATCH_WAVES) * ICP_ROW);
        }
        batch_reduce_rows(sh, nrows, per, g);
        // ---- K3: solve + compose (one lane)
        if (tid == 0) batch_solve(&sh, a.compose_mode, rules.svd_ieee);
        __syncthreads();
        if (sh.st.done != 0) break;                      // no pairs
        // ---- K4+K5: transform, error against the correspondences found before the update
        {
            float Rm[9], t[3];
#pragma unroll
            for (int i = 0; i < 9; i++) Rm[i] = sh.st.R[i];
#pragma unroll
            for (int i = 0; i < 3; i++) t[i] = sh.st.t[i];
#pragma unroll
            for (int r = 0; r < R; r++) {
                const float x = bx[pt[r]], y = by[pt[r]], z = bz[pt[r]];
                const float ox = ((Rm[0] * x + Rm[3] * y) + Rm[6] * z) + t[0];
                const float oy = ((Rm[1] * x + Rm[4] * y) + Rm[7] * z) + t[1];
                const float oz = ((Rm[2] * x + Rm[5] * y) + Rm[8] * z) + t[2];
                cx[r] = ox; cy[r] = oy; cz[r] = oz;
                if (!row_ok[r]) continue;
                float e0 = 0.f, e1 = 0.f;
                const bool mine = bidx[r] >= 0 && bidx[r] < p.m;
                const bool kept = rules.filter_pairs ? (__uint_as_float(dbits[r]) < a.max_distance_squared) : true;
                if (valid[r] && mine && kept) {
                    const float* q = after + 3 * (size_t)bidx[r];
                    const float dx = q[0] - ox, dy = q[1] - oy, dz = q[2] - oz;
                    e0 = (dx * dx + dy * dy) + dz * dz;  // diff.LengthSquared(), common.cpp:264-265
                    e1 = 1.f;
                }
                row_store_error(e0, e1, sh.rows + (row0 + r * BATCH_WAVES) * ICP_ROW);
            }
        }
        batch_reduce_rows(sh, nrows, per, g);
        // ---- K6: the stop rules
        if (tid == 0) batch_finalize(&sh, &rules);
        __syncthreads();
        if (sh.st.done != 0) break;
    }
}

template <bool FMA>
__global__ __launch_bounds__(BATCH_THREADS) void icp_batch_iterate_kernel(IcpBatchArgs a)
{
    __shared__ BatchShared sh;
    const IcpBatchProblem p = a.problems[blockIdx.x];
    IcpState* __restrict__ gst = a.states + blockIdx.x;
    if (gst->done != 0) return;                          // (uniform: the state is only written by this workgroup, in the launch before)
    constexpr int WORDS = (int)(sizeof(IcpState) / sizeof(int));
    static_assert(sizeof(IcpState) % sizeof(int) == 0, "the state block is copied word by word");
    for (int i = threadIdx.x; i < WORDS; i += BATCH_THREADS) reinterpret_cast<int*>(&sh.st)[i] = reinterpret_cast<const int*>(gst)[i];
    for (int i = threadIdx.x; i < BATCH_MAX_ROWS * ICP_ROW; i += BATCH_THREADS) sh.rows[i] = 0.0;
    __syncthreads();
    const int nrows = (p.n + ICP_ROW_POINTS - 1) / ICP_ROW_POINTS;
    const int per_lane = (nrows + BATCH_WAVES - 1) / BATCH_WAVES;
    if (per_lane <= 1) batch_run<1, FMA>(a, p, sh);
    else if (per_lane <= 2) batch_run<2, FMA>(a, p, sh);
    else if (per_lane <= 4) batch_run<4, FMA>(a, p, sh);
    else batch_run<8, FMA>(a, p, sh);
    __syncthreads();
    for (int i = threadIdx.x; i < WORDS; i += BATCH_THREADS) reinterpret_cast<int*>(gst)[i] = reinterpret_cast<const int*>(&sh.st)[i];
    if (threadIdx.x == 0 && sh.st.done == 0) atomicAdd(a.running, 1);
}

// ---------------------------------------------------------------------------------------------------------------
// host-side launchers
// ---------------------------------------------------------------------------------------------------------------
hipError_t icp_batch_prepare(const IcpBatchArgs& a, hipStream_t s)
{
    if (a.n_problems <= 0) return hipSuccess;
    hipLaunchKernelGGL(icp_batch_prepare_kernel, dim3(a.n_problems), dim3(BATCH_THREADS), 0, s, a);
    return hipGetLastError();
}

hipError_t icp_batch_iterate(const IcpBatchArgs& a, int fma, hipStream_t s)
{
    if (a.n_problems <= 0 || a.iters <= 0) return hipErrorInvalidValue;
    if (fma) hipLaunchKernelGGL(icp_batch_iterate_kernel<true>, dim3(a.n_problems), dim3(BATCH_THREADS), 0, s, a);
    else hipLaunchKernelGGL(icp_batch_iterate_kernel<false>, dim3(a.n_problems), dim3(BATCH_THREADS), 0, s, a);
    return hipGetLastError();
}

__global__ void preload_icp_batch_kernel() {}
hipError_t preload_icp_batch()
{
    hipFuncAttributes attr;
    return hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(preload_icp_batch_kernel));
}

}  // namespace mislam
