// K2-K6 -- everything of an ICP iteration that is not the nearest-neighbour search, for gfx950.
//
// One reference iteration (source/cuda-slam/icpcuda.cu:31-54) is ~10 thrust/cuBLAS/cuSOLVER passes over N-sized arrays
// with >= 10 host round trips.  Here it is four small kernels on one stream with NO host round trip:
//
//   K2  icp_moments_kernel          gather after[idx[i]] + count, sum b, sum a, sum a b^T in fp64 (one pass, nothing
//                                   materialised: replaces CalculateCentroid x4, GetAlignedCloud x2, the permutation
//                                   gather, GlmToCuBlas x2 and cublasSgemm of cudacommon.cu:168-201)
//   K3  icp_solve_kernel            fixed-order reduction of the block partials, 3x3 Jacobi SVD + Kabsch on one lane,
//                                   composition into the running transform (replaces cusolverDnSgesvd + 7 memcpys +
//                                   host glm code, cudacommon.cu:203-253, icpcuda.cu:35)
//   K4+K5 icp_transform_error_kernel  cur = R*before + t (TransformCloud, cudacommon.cu:132-136) fused with the squared
//                                   error against the correspondences found BEFORE the update (GetMeanSquaredError,
//                                   cudacommon.cu:138-148) and with re-arming the packed keys for the next search
//   K6  icp_finalize_kernel         error reduction + the stop rules of basicicp.cpp:52-57 / icpcuda.cu:40-53, evaluated
//                                   on the device: every kernel of later iterations returns at once when `done` is set.
//
// Since round 2 the default (cell-grid) search carries K2 and K4+K5 itself (nn_grid.hip: the fused iteration); the stand-alone
// kernels below serve the every-pair search, the multi-GPU split of the fixed cloud, MI_SUM_CPU_SEQUENTIAL and the test-grade
// primitives.  Either way an iteration's sums are "rows" (icp_rows.hpp): one row of 18 partial sums per 64 moving points, added
// in one fixed tree -- so every strategy yields the same bits -- then icp_rows_reduce (<= 64 workgroups) and the solve kernel
// sum the rows in index order.  No float atomics: results are bitwise reproducible run to run.
// The stop rule of iteration i is evaluated at the START of the solve kernel of iteration i+1 (its error sums ride in the same
// rows as that iteration's moments), or by icp_finalize_pending when the host stops enqueuing: one all-reduce per iteration on
// several GPUs, two launches per iteration on one (the search, then the rows reduction whose last workgroup solves).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "icp_rows.hpp"
#include "icp_solve.hpp"
#include "kernels.h"
#include "reduce.hpp"
#include "svd3.hpp"

namespace mislam {

__global__ __launch_bounds__(256) void fill_keys_kernel(unsigned long long* __restrict__ keys, int n)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) keys[i] = KEY_INIT;
}

// AoS xyz (12 B/point, the reference's host layout) -> SoA x[], y[], z[] (+ optional float4 copy for gathers).
// Entries [n, n_pad) replicate point n-1 (see K1's padding rule).
__global__ __launch_bounds__(256) void aos_to_soa_kernel(const float* __restrict__ aos, int n, int n_pad, float* __restrict__ x,
                                                         float* __restrict__ y, float* __restrict__ z, float4* __restrict__ packed)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_pad) return;
    const int s = i < n ? i : n - 1;
    const float px = aos[3 * (size_t)s], py = aos[3 * (size_t)s + 1], pz = aos[3 * (size_t)s + 2];
    x[i] = px; y[i] = py; z[i] = pz;
    if (packed != nullptr) packed[i] = make_float4(px, py, pz, 0.f);
}

__global__ __launch_bounds__(256) void soa_to_aos_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                         const float* __restrict__ z, int n, float* __restrict__ aos)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    aos[3 * (size_t)i] = x[i]; aos[3 * (size_t)i + 1] = y[i]; aos[3 * (size_t)i + 2] = z[i];
}

// keys -> idx[], d2[] (test-grade mi_nn_search output).  keys[s] belongs to sorted slot s; order[s] (may be null) is the
// caller's index of that slot.
__global__ __launch_bounds__(256) void unpack_keys_kernel(const unsigned long long* __restrict__ keys, const int* __restrict__ order,
                                                          int n, int* __restrict__ idx, float* __restrict__ d2)
{
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= n) return;
    const unsigned long long k = keys[s];
    const int i = order != nullptr ? order[s] : s;
    idx[i] = (int)(unsigned int)(k & 0xffffffffull);
    if (d2 != nullptr) d2[i] = __uint_as_float((unsigned int)(k >> 32));
}

// idx[] (+ optional keep mask) -> keys with d2 = 0 for kept pairs and +inf for dropped ones, so the ICP kernels can be
// driven from caller-supplied correspondences (mi_kabsch / mi_transform_mse).
__global__ __launch_bounds__(256) void pack_keys_kernel(const int* __restrict__ idx, const unsigned char* __restrict__ keep, int n,
                                                        unsigned long long* __restrict__ keys)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const bool k = keep == nullptr || keep[i] != 0;
    const unsigned int hi = k ? 0u : 0x7f800000u;
    keys[i] = ((unsigned long long)hi << 32) | (unsigned int)idx[i];
}

// ---------------------------------------------------------------------------------------------------------------
// K2: fused moments.  acc = { count, sum b (3), sum a (3), sum a_r b_c (9, row-major in r) }
// A pair is used when its winner lies in this device's target shard [shard_lo, shard_hi) -- so in the multi-GPU path
// every pair is accumulated by exactly one rank, the one that owns the target's coordinates -- and, with filter_pairs,
// when d2 < max_distance_squared (common.cpp:490).
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(ICP_ROW_POINTS) void icp_moments_rows_kernel(IcpView v, double* __restrict__ rows)
{
    if (v.state->done != 0) return;
    const int i = blockIdx.x * ICP_ROW_POINTS + threadIdx.x;
    bool use = false;
    float bx = 0.f, by = 0.f, bz = 0.f;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i < v.n) {
        const unsigned long long key = v.keys[i];
        const int gidx = (int)(unsigned int)(key & 0xffffffffull);
        const float d2 = __uint_as_float((unsigned int)(key >> 32));
        const bool mine = gidx >= v.shard_lo && gidx < v.shard_hi;
        const bool kept = v.filter_pairs ? (d2 < v.max_distance_squared) : true;
        if (mine && kept) {
            a = v.tgt4[gidx - v.shard_lo];
            bx = v.cx[i]; by = v.cy[i]; bz = v.cz[i];
            use = true;
        }
    }
    row_store_pair_moments(use, bx, by, bz, a.x, a.y, a.z, rows + (size_t)blockIdx.x * ICP_ROW);     // (the one producer of moments rows: icp_rows.hpp)
}

// rows [first, first + count) of ICP_ROW doubles -> out[blockIdx.x] : workgroup g sums its contiguous slice of rows in index
// order (56 strips of rows, then the strips in order)
// While it is at it, the kernel also deals the NEXT search its work order (sched != null): chunks whose wave walked the box
// hierarchy in this iteration -- they will again, the flags move slowly -- go to the front, so that those long walks start at once
// and the short grid-only chunks fill in behind them instead of the other way round (a wave that walks lives ~5x longer).  Scheduling
// only: which workgroup handles which chunk never changes a result.
constexpr int ROWS_REDUCE_THREADS = 1024;
constexpr int ROWS_REDUCE_STRIPS = ROWS_REDUCE_THREADS / ICP_ROW;      // 56 strips of rows, 18 columns each

// a dealing workgroup: the chunks of rows [lo, hi) into the next search's order, walking ones from the front, the others from the back
__device__ __forceinline__ void deal_work_order(const IcpSchedule& sched, int* cursors, int lo, int hi, int nrows)
{
    __shared__ int s_far, s_near, s_base_far, s_base_near;
    if (threadIdx.x == 0) { s_far = 0; s_near = 0; }
    __syncthreads();
    // two passes over the slice: count, reserve a range at each end of the order, place
    int my_far = 0, my_near = 0;
    for (int r = lo + (int)threadIdx.x; r < hi; r += ROWS_REDUCE_THREADS) { if (sched.far[r]) my_far++; else my_near++; }
    if (my_far) atomicAdd(&s_far, my_far);
    if (my_near) atomicAdd(&s_near, my_near);
    __syncthreads();
    if (threadIdx.x == 0) {
        s_base_far = atomicAdd(&cursors[0], s_far);
        s_base_near = atomicAdd(&cursors[1], s_near);
        s_far = 0; s_near = 0;
    }
    __syncthreads();
    for (int r0 = lo; r0 < hi; r0 += ROWS_REDUCE_THREADS) {    // one LDS cursor per class
        const int r = r0 + (int)threadIdx.x;
        if (r < hi) {
            if (sched.far[r]) sched.order[s_base_far + atomicAdd(&s_far, 1)] = r;
            else sched.order[nrows - 1 - (s_base_near + atomicAdd(&s_near, 1))] = r;
        }
    }
}

// a summing workgroup: rows [lo, hi) -> out_row[0..18), 56 strips of rows first, then the strips in order (lds: ROWS_REDUCE_STRIPS * ICP_ROW doubles)
__device__ __forceinline__ void sum_row_slice(const double* __restrict__ rows, int lo, int hi, double* lds, double* out_row)
{
    const int k = threadIdx.x % ICP_ROW, strip = threadIdx.x / ICP_ROW;
    if (strip < ROWS_REDUCE_STRIPS) {
        double s = 0.0;
#pragma unroll 4
        for (int r = lo + strip; r < hi; r += ROWS_REDUCE_STRIPS) s += rows[(size_t)r * ICP_ROW + k];
        lds[strip * ICP_ROW + k] = s;
    }
    __syncthreads();
    if (threadIdx.x < ICP_ROW) {
        double tot = lds[threadIdx.x];
        for (int g = 1; g < ROWS_REDUCE_STRIPS; g++) tot += lds[g * ICP_ROW + threadIdx.x];
        out_row[threadIdx.x] = tot;
    }
}

// The two jobs are independent, so with a schedule the launch is twice as wide: workgroups [0, n_sum) add their slices up, workgroups
// [n_sum, 2 n_sum) deal the next search its order for theirs -- the launch lasts as long as the longer of the two, not as their sum.
__global__ __launch_bounds__(ROWS_REDUCE_THREADS) void icp_rows_reduce_kernel(const double* __restrict__ rows, int nrows, int rows_per_block,
                                                                             double* __restrict__ out, IcpSchedule sched, int n_sum)
{
    __shared__ double lds[ROWS_REDUCE_STRIPS * ICP_ROW];
    const int slice = (int)blockIdx.x >= n_sum ? (int)blockIdx.x - n_sum : (int)blockIdx.x;
    const int lo = slice * rows_per_block;
    const int hi = lo + rows_per_block < nrows ? lo + rows_per_block : nrows;
    if ((int)blockIdx.x >= n_sum) deal_work_order(sched, sched.counters, lo, hi, nrows);
    else sum_row_slice(rows, lo, hi, lds, out + (size_t)blockIdx.x * ICP_ROW);
}

// The same launch with the deferred solve behind it (one rank, above ICP_FUSED_SOLVE_MAX_ROWS): the summing workgroup that finishes LAST goes
// on as icp_solve_deferred_kernel would.  Every summing workgroup writes its row exactly as above, releases it at agent scope and draws a ticket;
// whoever draws n_sum - 1 knows all n_sum rows are out, acquires, and its first wave reads them back FROM MEMORY (its own row too) and runs
// solve_deferred_wave: the same rows in the same butterfly, so the same bits as the two-launch form.  Nobody waits for anybody -- a workgroup that
// is not last returns -- so the launch needs no co-residency and cannot hang.  The last arrival leaves the ticket at 0 for the next launch.
// The dealing workgroups take no ticket.  Their two cursors come in two pairs: this launch deals on pair `parity` (the step's parity, from the host),
// and the solving wave zeroes the OTHER pair, which no workgroup of this launch touches and the next launch deals on; the pair in use is zeroed by
// the next launch's solving wave, a launch boundary behind the last dealer.  (icp_solve_deferred_kernel zeroes both: no dealer runs beside it.)
__global__ __launch_bounds__(ROWS_REDUCE_THREADS) void icp_rows_reduce_solve_kernel(IcpState* __restrict__ state, const double* __restrict__ rows, int nrows,
                                                                                   int rows_per_block, double* out, IcpSchedule sched, int n_sum, int parity,
                                                                                   int* ticket, int compose_mode, IcpRules rules, int mark_pending)
{
    __shared__ double lds[ROWS_REDUCE_STRIPS * ICP_ROW];
    __shared__ double sums[ICP_ROW];
    __shared__ int s_ticket;
    const int slice = (int)blockIdx.x >= n_sum ? (int)blockIdx.x - n_sum : (int)blockIdx.x;
    const int lo = slice * rows_per_block;
    const int hi = lo + rows_per_block < nrows ? lo + rows_per_block : nrows;
    if ((int)blockIdx.x >= n_sum) { deal_work_order(sched, sched.counters + 2 * parity, lo, hi, nrows); return; }
    sum_row_slice(rows, lo, hi, lds, out + (size_t)blockIdx.x * ICP_ROW);
    if (threadIdx.x == 0) {              // (the row's 18 stores are this wave's: its wait covers them)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        s_ticket = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    if (s_ticket != n_sum - 1 || threadIdx.x >= 64) return;      // not the last arrival; of the last one, the first wave goes on alone
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    if (threadIdx.x == 0) __hip_atomic_store(ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (sched.counters != nullptr && threadIdx.x < 2) sched.counters[2 * (1 - parity) + threadIdx.x] = 0;
    if (state->done != 0) return;
    solve_deferred_wave(state, out, n_sum, sums, compose_mode, rules, mark_pending);
}

// reduced rows -> state->mom[16], state->err[2] (contiguous in the state block); which = 1 moments, 2 error sums, 3 both
__global__ __launch_bounds__(64) void icp_rows_to_state_kernel(IcpState* __restrict__ state, const double* __restrict__ part, int count, int which)
{
    if (state->done != 0) return;
    __shared__ double sums[ICP_ROW];
    reduce_rows_wave(part, count, sums);
    if (threadIdx.x >= ICP_ROW) return;
    const double tot = sums[threadIdx.x];
    if (threadIdx.x < ICP_MOMENTS) { if (which & 1) state->mom[threadIdx.x] = tot; }
    else if (which & 2) state->err[threadIdx.x - ICP_MOMENTS] = tot;
}

// ---------------------------------------------------------------------------------------------------------------
// K3: solve + compose (one lane).  partials == nullptr: the moments are already in state->mom (multi-GPU path).
// (reduce_rows_wave, solve_from_moments, apply_solve: icp_solve.hpp, shared with icp_batch.hip)
// ---------------------------------------------------------------------------------------------------------------

// ---------------------------------------------------------------------------------------------------------------
// K4+K5: cur = R*before + t for ALL n_pad entries (padding stays a copy of a real point), squared error of the kept pairs
// against the OLD correspondences (basicicp.cpp:48, icpcuda.cu:38), keys re-armed for the next search.
// err partial = { sum |a - cur|^2, kept pairs }
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(ICP_ROW_POINTS) void icp_transform_error_rows_kernel(IcpView v, double* __restrict__ rows, int rearm)
{
    if (v.state->done != 0) return;
    float R[9], t[3];
#pragma unroll
    for (int i = 0; i < 9; i++) R[i] = v.state->R[i];
#pragma unroll
    for (int i = 0; i < 3; i++) t[i] = v.state->t[i];
    float e0 = 0.f, e1 = 0.f;
    const int i = blockIdx.x * ICP_ROW_POINTS + threadIdx.x;
    if (i < v.n_pad) {
        const float x = v.bx[i], y = v.by[i], z = v.bz[i];
        // TransformPoint: (rotationMatrix * point) + translationVector  (common.cpp:45-49), glm operation order
        const float ox = ((R[0] * x + R[3] * y) + R[6] * z) + t[0];
        const float oy = ((R[1] * x + R[4] * y) + R[7] * z) + t[1];
        const float oz = ((R[2] * x + R[5] * y) + R[8] * z) + t[2];
        v.cx[i] = ox; v.cy[i] = oy; v.cz[i] = oz;
        if (i < v.n) {
            const unsigned long long key = v.keys[i];
            const int gidx = (int)(unsigned int)(key & 0xffffffffull);
            const float d2 = __uint_as_float((unsigned int)(key >> 32));
            const bool mine = gidx >= v.shard_lo && gidx < v.shard_hi;
            const bool kept = v.filter_pairs ? (d2 < v.max_distance_squared) : true;
            unsigned long long next_key = KEY_INIT;
            float resid = 0.f;
            if (mine) {
                const float4 a = v.tgt4[gidx - v.shard_lo];
                const float dx = a.x - ox, dy = a.y - oy, dz = a.z - oz;
                const float e = (dx * dx + dy * dy) + dz * dz;       // diff.LengthSquared(), common.cpp:264-265
                if (kept) {
                    e0 = e;
                    e1 = 1.f;
                    resid = e;
                }
                // The old match under the new transform is a real candidate of the next search, evaluated with the
                // search's own arithmetic, so its key is a valid starting bound.
                const float c = v.fma ? __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx)) : e;
                next_key = ((unsigned long long)__float_as_uint(c) << 32) | (unsigned int)gidx;
            }
            if (rearm == 1) v.keys[i] = KEY_INIT;
            else if (rearm == 2) v.keys[i] = next_key;
            if (v.resid != nullptr) v.resid[i] = resid;
        }
    }
    row_store_error(e0, e1, rows + (size_t)blockIdx.x * ICP_ROW);
}

// ---------------------------------------------------------------------------------------------------------------
// MI_SUM_CPU_SEQUENTIAL: cpu-slam's running sums, bit for bit.
// cpu-slam accumulates its centroids and its error with ONE sequential fp32 running sum each (std::accumulate over Point_f,
// common.cpp:281-284; `diffSum +=`, :259-268), in the order of the kept pairs = the caller's point order.  At 2e4 points the
// centroid is already 1.3e-4 off the exact mean, and the error feeds the stop rule -- so retracing cpu-slam's trajectory
// beyond bunny size needs these very roundings.  A sequential fp32 sum cannot be re-associated, but it can be fed fast:
// one wave per running sum, 64 terms gathered per step by the 64 lanes (in the caller's order, through inv_order), then
// added one by one from lane registers via v_readlane.  A dropped pair contributes +0.0f, which leaves an fp32 sum
// unchanged, so no flags are needed.  ~8 cycles per term: 3.3 ms per million points, paid only in this mode.
// ---------------------------------------------------------------------------------------------------------------
// 6 waves: wave w < 3 sums component w of the kept moving points, wave w >= 3 component w-3 of their matched fixed points
__global__ __launch_bounds__(384) void icp_seq_centroid_kernel(IcpView v)
{
    if (v.state->done != 0) return;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float acc = 0.f;
    for (int i0 = 0; i0 < v.n; i0 += 64) {
        const int i = i0 + lane;
        float term = 0.f;
        if (i < v.n) {
            const int s = v.inv_order[i];
            const unsigned long long key = v.keys[s];
            const int gidx = (int)(unsigned int)(key & 0xffffffffull);
            const float d2 = __uint_as_float((unsigned int)(key >> 32));
            const bool kept = v.filter_pairs ? (d2 < v.max_distance_squared) : true;
            if (kept) {
                if (wave < 3) term = wave == 0 ? v.cx[s] : (wave == 1 ? v.cy[s] : v.cz[s]);
                else {
                    const float4 a = v.tgt4[gidx - v.shard_lo];
                    term = wave == 3 ? a.x : (wave == 4 ? a.y : a.z);
                }
            }
        }
        acc = seq_add64(acc, term);
    }
    if (lane == 0) {
        if (wave < 3) v.state->seq_sum_b[wave] = acc;
        else v.state->seq_sum_a[wave - 3] = acc;
    }
}

__global__ __launch_bounds__(64) void icp_seq_error_kernel(IcpView v)
{
    if (v.state->done != 0) return;
    const int lane = threadIdx.x & 63;
    float acc = 0.f;
    for (int i0 = 0; i0 < v.n; i0 += 64) {
        const int i = i0 + lane;
        const float term = i < v.n ? v.resid[v.inv_order[i]] : 0.f;
        acc = seq_add64(acc, term);
    }
    if (lane == 0) v.state->seq_sum_err = acc;
}

__global__ __launch_bounds__(256) void invert_order_kernel(const int* __restrict__ order, int n, int* __restrict__ inv)
{
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s < n) inv[order[s]] = s;
}

// ---------------------------------------------------------------------------------------------------------------
// K6: error + stop rules.  (finalize_iteration: icp_solve.hpp)
// ---------------------------------------------------------------------------------------------------------------

// ---------------------------------------------------------------------------------------------------------------
// K3 + K6: the deferred solve.  An iteration's error sums arrive together with the NEXT iteration's moments (same rows), so the
// solve kernel first settles the previous iteration's stop rule (err_pending) and, if it fired, applies nothing -- that
// iteration's search and moments were in vain, once per registration.  part != null: the sums are the `count` reduced rows;
// part == null: they are already in state->mom / state->err (multi-GPU: all-reduced there).
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void icp_solve_deferred_kernel(IcpState* __restrict__ state, const double* __restrict__ part, int count,
                                                                int compose_mode, IcpRules rules, int mark_pending, int* __restrict__ sched_counters)
{
    // the reduce kernel's range cursors (IcpSchedule), both pairs: no dealing workgroup runs beside this launch
    if (sched_counters != nullptr && threadIdx.x < ICP_SCHED_CURSORS) sched_counters[threadIdx.x] = 0;
    if (state->done != 0) return;
    __shared__ double sums[ICP_ROW];
    solve_deferred_wave(state, part, count, sums, compose_mode, rules, mark_pending);
}

// the same evaluation alone, when the host stops enqueuing and wants the state
__global__ __launch_bounds__(64) void icp_finalize_pending_kernel(IcpState* __restrict__ state, const double* __restrict__ part, int count, IcpRules rules)
{
    if (state->done != 0 || !state->err_pending) return;
    __shared__ double sums[ICP_ROW];
    if (part != nullptr) reduce_rows_wave(part, count, sums);
    else {
        if (threadIdx.x < ICP_ROW) sums[threadIdx.x] = threadIdx.x < ICP_MOMENTS ? 0.0 : state->err[threadIdx.x - ICP_MOMENTS];
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    state->err_pending = 0;
    state->err[0] = sums[ICP_MOMENTS];
    state->err[1] = sums[ICP_MOMENTS + 1];
    finalize_iteration(state, sums[ICP_MOMENTS], sums[ICP_MOMENTS + 1], rules);
}

__global__ void icp_mark_pending_kernel(IcpState* __restrict__ state)
{
    if (threadIdx.x == 0 && state->done == 0) state->err_pending = 1;
}

// ---------------------------------------------------------------------------------------------------------------
// host-side launchers
// ---------------------------------------------------------------------------------------------------------------
int icp_row_count(int n) { return (n + ICP_ROW_POINTS - 1) / ICP_ROW_POINTS; }

static_assert(ICP_REDUCED_ROWS == ICP_MAX_REDUCED_ROWS, "kernels.h and icp_rows.hpp agree");
int icp_reduced_count(int nrows)
{
    int g = (nrows + 31) / 32;           // at least ~32 rows per workgroup
    if (g > ICP_MAX_REDUCED_ROWS) g = ICP_MAX_REDUCED_ROWS;
    return g < 1 ? 1 : g;
}

// all_rows: write every one of the ICP_REDUCED_ROWS output rows, the ones past this cloud's own count as zeros (their workgroups find an
// empty slice).  The multi-GPU path all-reduces the 64 rows IN PLACE: a rank whose share yields fewer rows than a neighbour's would
// otherwise keep the neighbour's summed rows from the previous iteration and add them into the next collective.
hipError_t icp_rows_reduce(const double* rows, int nrows, double* part, hipStream_t s, const IcpSchedule* sched, bool all_rows, int parity)
{
    const int g = icp_reduced_count(nrows);
    const int per = (nrows + g - 1) / g;
    const int n_sum = all_rows ? ICP_REDUCED_ROWS : g;
    IcpSchedule sc{};
    if (sched != nullptr) sc = *sched;
    if (sc.counters != nullptr) sc.counters += 2 * (parity & 1);     // (the pair of cursors this step deals on)
    hipLaunchKernelGGL(icp_rows_reduce_kernel, dim3(sched != nullptr && sc.order != nullptr ? 2 * n_sum : n_sum), dim3(ROWS_REDUCE_THREADS), 0, s, rows, nrows, per, part, sc, n_sum);
    return hipGetLastError();
}

hipError_t icp_rows_reduce_solve(IcpState* state, const double* rows, int nrows, double* part, const IcpSchedule* sched, int parity, int* ticket,
                                 int compose_mode, const IcpRules& rules, int mark_pending, hipStream_t s)
{
    if (ticket == nullptr) return hipErrorInvalidValue;
    const int g = icp_reduced_count(nrows);
    const int per = (nrows + g - 1) / g;
    IcpSchedule sc{};
    if (sched != nullptr && sched->order != nullptr) sc = *sched;
    hipLaunchKernelGGL(icp_rows_reduce_solve_kernel, dim3(sc.order != nullptr ? 2 * g : g), dim3(ROWS_REDUCE_THREADS), 0, s, state, rows, nrows, per, part, sc, g,
                       parity & 1, ticket, compose_mode, rules, mark_pending);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void icp_schedule_reset_kernel(IcpSchedule sched, int nrows)
{
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r < nrows) { sched.order[r] = r; sched.far[r] = 0; if (sched.lanes != nullptr) sched.lanes[r] = 0ull; }
    if (r < ICP_SCHED_CURSORS) sched.counters[r] = 0;
    if (r == 0 && sched.ticket != nullptr) *sched.ticket = 0;
}

hipError_t icp_schedule_reset(const IcpSchedule& sched, int nrows, hipStream_t s)
{
    hipLaunchKernelGGL(icp_schedule_reset_kernel, dim3((nrows + 255) / 256 > 0 ? (nrows + 255) / 256 : 1), dim3(256), 0, s, sched, nrows);
    return hipGetLastError();
}

hipError_t icp_rows_to_state(IcpState* state, const double* part, int count, int which, hipStream_t s)
{
    hipLaunchKernelGGL(icp_rows_to_state_kernel, dim3(1), dim3(64), 0, s, state, part, count, which);
    return hipGetLastError();
}

// Small clouds (round 4): rows reduce AND deferred solve in ONE workgroup -- below ~10^5 points an ICP step is three launches of which the
// search is 60 %, and what the two others cost is mostly being launches.  Thread (b, k) walks what workgroup b's column k of
// icp_rows_reduce_kernel adds up -- the same strips, the same order, so the same 64 (or fewer) rows to the last bit -- into LDS, and the first
// wave goes on exactly as icp_solve_deferred_kernel does.  No work order is dealt: every wave of such a search is resident from the start.
__global__ __launch_bounds__(ROWS_REDUCE_THREADS) void icp_reduce_solve_kernel(IcpState* __restrict__ state, const double* __restrict__ rows, int nrows,
                                                                              int rows_per_block, int count, int compose_mode, IcpRules rules, int mark_pending)
{
    if (state->done != 0) return;
    constexpr int STRIPS = ROWS_REDUCE_THREADS / ICP_ROW;
    __shared__ double part[ICP_REDUCED_ROWS * ICP_ROW];
    __shared__ double sums[ICP_ROW];
    // (a slice here has at most FUSED_SLICE <= STRIPS rows, i.e. every strip of the two-launch form holds at most one row: its sum is
    // 0.0 + that row, and the strips are added in order -- the loads first, all in flight together, then the chain of additions)
    constexpr int FUSED_SLICE = ICP_FUSED_SOLVE_MAX_ROWS / ICP_REDUCED_ROWS;
    static_assert(FUSED_SLICE <= STRIPS, "one row per strip");
    for (int item = (int)threadIdx.x; item < count * ICP_ROW; item += ROWS_REDUCE_THREADS) {
        const int b = item / ICP_ROW, k = item - b * ICP_ROW;
        const int lo = b * rows_per_block;
        const int hi = lo + rows_per_block < nrows ? lo + rows_per_block : nrows;
        double val[FUSED_SLICE];
#pragma unroll
        for (int j = 0; j < FUSED_SLICE; j++) val[j] = rows[(size_t)min(lo + j, nrows - 1) * ICP_ROW + k];     // (unconditional: all in flight at once)
#pragma unroll
        for (int j = 0; j < FUSED_SLICE; j++) val[j] = lo + j < hi ? val[j] : 0.0;
        double tot = 0.0 + val[0];
#pragma unroll
        for (int j = 1; j < FUSED_SLICE; j++) tot = tot + (0.0 + val[j]);       // (an empty strip adds its 0.0, as it does there)
        if (FUSED_SLICE < STRIPS) tot = tot + 0.0;
        part[item] = tot;
    }
    __syncthreads();
    if (threadIdx.x >= 64) return;                   // the first wave goes on alone (the barrier inside reduce_rows_wave then counts one wave)
    solve_deferred_wave(state, part, count, sums, compose_mode, rules, mark_pending);
}
hipError_t icp_reduce_solve(IcpState* state, const double* rows, int nrows, int compose_mode, const IcpRules& rules, int mark_pending, hipStream_t s)
{
    const int g = icp_reduced_count(nrows);
    const int per = (nrows + g - 1) / g;
    if (nrows > ICP_FUSED_SOLVE_MAX_ROWS || per > ICP_FUSED_SOLVE_MAX_ROWS / ICP_REDUCED_ROWS) return hipErrorInvalidValue;   // (a slice must fit the kernel's registers)
    hipLaunchKernelGGL(icp_reduce_solve_kernel, dim3(1), dim3(ROWS_REDUCE_THREADS), 0, s, state, rows, nrows, per, g, compose_mode, rules, mark_pending);
    return hipGetLastError();
}

hipError_t icp_solve_deferred(IcpState* state, const double* part, int count, int compose_mode, const IcpRules& rules, int mark_pending, hipStream_t s,
                              int* sched_counters)
{
    hipLaunchKernelGGL(icp_solve_deferred_kernel, dim3(1), dim3(64), 0, s, state, part, count, compose_mode, rules, mark_pending, sched_counters);
    return hipGetLastError();
}

hipError_t icp_finalize_pending(IcpState* state, const double* part, int count, const IcpRules& rules, hipStream_t s)
{
    hipLaunchKernelGGL(icp_finalize_pending_kernel, dim3(1), dim3(64), 0, s, state, part, count, rules);
    return hipGetLastError();
}

hipError_t icp_mark_pending(IcpState* state, hipStream_t s)
{
    hipLaunchKernelGGL(icp_mark_pending_kernel, dim3(1), dim3(64), 0, s, state);
    return hipGetLastError();
}

static inline int blocks_for(int n, int cap)
{
    int b = (n + 255) / 256;
    if (b > cap) b = cap;
    if (b < 1) b = 1;
    return b;
}

__global__ __launch_bounds__(256) void deal_chunks_kernel(const float* __restrict__ sx, const float* __restrict__ sy, const float* __restrict__ sz,
                                                          int n_all, int rank, int world, int n_local, int n_pad, float* __restrict__ dx,
                                                          float* __restrict__ dy, float* __restrict__ dz)
{
    static_assert(ICP_CHUNK_POINTS == ICP_ROW_POINTS, "a dealt chunk is one row of partial sums");
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_pad) return;
    const int il = i < n_local ? i : n_local - 1;
    const long long g = ((long long)(il / ICP_CHUNK_POINTS) * world + rank) * ICP_CHUNK_POINTS + il % ICP_CHUNK_POINTS;
    const int j = g < n_all ? (int)g : n_all - 1;
    dx[i] = sx[j]; dy[i] = sy[j]; dz[i] = sz[j];
}

hipError_t deal_chunks_soa(const float* sx, const float* sy, const float* sz, int n_all, int rank, int world, int n_local, int n_pad,
                           float* dx, float* dy, float* dz, hipStream_t s)
{
    if (n_pad <= 0) return hipSuccess;
    hipLaunchKernelGGL(deal_chunks_kernel, dim3((n_pad + 255) / 256), dim3(256), 0, s, sx, sy, sz, n_all, rank, world, n_local, n_pad, dx, dy, dz);
    return hipGetLastError();
}

hipError_t fill_keys(unsigned long long* keys, int n, hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(fill_keys_kernel, dim3((n + 255) / 256), dim3(256), 0, s, keys, n);
    return hipGetLastError();
}

hipError_t aos_to_soa(const float* aos, int n, int n_pad, float* x, float* y, float* z, float4* packed, hipStream_t s)
{
    if (n_pad <= 0) return hipSuccess;
    hipLaunchKernelGGL(aos_to_soa_kernel, dim3((n_pad + 255) / 256), dim3(256), 0, s, aos, n, n_pad, x, y, z, packed);
    return hipGetLastError();
}

hipError_t soa_to_aos(const float* x, const float* y, const float* z, int n, float* aos, hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(soa_to_aos_kernel, dim3((n + 255) / 256), dim3(256), 0, s, x, y, z, n, aos);
    return hipGetLastError();
}

hipError_t unpack_keys(const unsigned long long* keys, const int* order, int n, int* idx, float* d2, hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(unpack_keys_kernel, dim3((n + 255) / 256), dim3(256), 0, s, keys, order, n, idx, d2);
    return hipGetLastError();
}

hipError_t pack_keys(const int* idx, const unsigned char* keep, int n, unsigned long long* keys, hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(pack_keys_kernel, dim3((n + 255) / 256), dim3(256), 0, s, idx, keep, n, keys);
    return hipGetLastError();
}

int icp_reduce_blocks(int n) { return blocks_for(n, ICP_MAX_PARTIAL_BLOCKS); }

hipError_t icp_moments_rows(const IcpView& v, double* rows, hipStream_t s)
{
    hipLaunchKernelGGL(icp_moments_rows_kernel, dim3(icp_row_count(v.n)), dim3(ICP_ROW_POINTS), 0, s, v, rows);
    return hipGetLastError();
}

hipError_t invert_order(const int* order, int n, int* inv, hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(invert_order_kernel, dim3((n + 255) / 256), dim3(256), 0, s, order, n, inv);
    return hipGetLastError();
}

// cpu-slam's cross-covariance (LeastSquaresSVD, common.cpp:525-530): the kept pairs centred with ITS centroids -- the sequential sums just taken, divided
// by (float)count -- in fp32, as GetAlignedCloud does, then alignedAfter * alignedBefore^T.  The products are summed in fp64 like the restatement's
// (oracle/slam_oracle.c oracle_least_squares_svd: Eigen's fp32 GEMM blocking is machine-dependent), thread t taking pairs t, t + 1024, ... and the threads'
// sums added in one fixed tree: another grouping of the same doubles than the restatement's index order -- 1e-16 relative, below the fp32 cast.  One
// workgroup: the mode's cost is irrelevant.
__global__ __launch_bounds__(1024) void icp_seq_cross_kernel(IcpView v)
{
    if (v.state->done != 0) return;
    __shared__ double part[1024];
    __shared__ int s_count;
    // the count of kept pairs (the centroids' divisor): counted here in the same pass order
    int kept_n = 0;
    for (int i = threadIdx.x; i < v.n; i += 1024) {
        const float d2 = __uint_as_float((unsigned int)(v.keys[i] >> 32));
        kept_n += (v.filter_pairs ? (d2 < v.max_distance_squared) : true) ? 1 : 0;
    }
    if (threadIdx.x == 0) s_count = 0;
    __syncthreads();
    atomicAdd(&s_count, kept_n);
    __syncthreads();
    const float fn = (float)s_count;
    float cb[3], ca[3];
    for (int d = 0; d < 3; d++) { cb[d] = v.state->seq_sum_b[d] / fn; ca[d] = v.state->seq_sum_a[d] / fn; }     // common.cpp:283
    double acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = threadIdx.x; i < v.n; i += 1024) {
        const unsigned long long key = v.keys[i];
        const float d2 = __uint_as_float((unsigned int)(key >> 32));
        if (!(v.filter_pairs ? (d2 < v.max_distance_squared) : true)) continue;
        const int gidx = (int)(unsigned int)(key & 0xffffffffull);
        const float4 a = v.tgt4[gidx - v.shard_lo];
        const float ab[3] = {v.cx[i] - cb[0], v.cy[i] - cb[1], v.cz[i] - cb[2]};        // GetAlignedCloud: point - center, fp32
        const float aa[3] = {a.x - ca[0], a.y - ca[1], a.z - ca[2]};
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++) acc[3 * r + c] += (double)aa[r] * (double)ab[c];
    }
    for (int q = 0; q < 9; q++) {
        part[threadIdx.x] = acc[q];
        __syncthreads();
        for (int w = 512; w > 0; w >>= 1) {
            if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
            __syncthreads();
        }
        if (threadIdx.x == 0) v.state->seq_H[q] = (float)part[0];
        __syncthreads();
    }
}

hipError_t icp_seq_centroids(const IcpView& v, hipStream_t s)
{
    hipLaunchKernelGGL(icp_seq_centroid_kernel, dim3(1), dim3(384), 0, s, v);
    hipLaunchKernelGGL(icp_seq_cross_kernel, dim3(1), dim3(1024), 0, s, v);      // (reads the sums the kernel before it left in the state)
    return hipGetLastError();
}

hipError_t icp_seq_error(const IcpView& v, hipStream_t s)
{
    hipLaunchKernelGGL(icp_seq_error_kernel, dim3(1), dim3(64), 0, s, v);
    return hipGetLastError();
}

hipError_t icp_transform_error_rows(const IcpView& v, double* rows, int rearm, hipStream_t s)
{
    hipLaunchKernelGGL(icp_transform_error_rows_kernel, dim3(icp_row_count(v.n_pad)), dim3(ICP_ROW_POINTS), 0, s, v, rows, rearm);
    return hipGetLastError();
}

}  // namespace mislam

// Touching one kernel of this translation unit makes the runtime load its code object now (mi_ctx_create) instead of at the
// first launch inside a registration call (deferred loading: 5-16 ms per object, once).
namespace mislam {
__global__ void preload_icp_kernels_kernel() {}
hipError_t preload_icp_kernels()
{
    hipFuncAttributes attr;
    return hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(preload_icp_kernels_kernel));
}
}  // namespace mislam
