// Fast-Gauss-Transform E-step of rigid CPD on gfx950: the reference's approximation-type "full" / "hybrid"
// (source/common/fgt.cpp, source/common/cpdutils.cpp:19-77; both of its builds run this part on the CPU).
//
// The transform is  v(q) = sum_i w_i exp(-|q - s_i|^2 / sigma^2):  the sources s are grouped into K cells by greedy
// farthest-point clustering, each cell keeps the p-truncated Hermite/Taylor coefficients of its sources about the cell mean
// (pd = C(p+2,3) of them), and a query sums, over the cells within sqrt(e)*sigma, one polynomial of degree < p.
//
//   kcenter   ONE workgroup of 1024 lanes: the farthest-point sweep is a chain of K dependent arg-max steps, so it is
//             latency-bound; points, distances and labels live in registers (<= 16 per lane) and the arg-max travels with
//             the winner's coordinates through DPP-free shuffles + one LDS exchange, one barrier per step.  Same arithmetic,
//             same first-maximum tie rule and same strict-< relabel rule as the reference, so the labels are identical.
//             Clouds beyond 16 384 points: several workgroups in one cooperative launch, each with its share in registers and the arg-max
//             through memory behind a ticket barrier (fgt_kcenter_coop_kernel, round 5), or one workgroup with its distances in memory /
//             two launches per centre (the later E-steps' few additional centres); a sweep can be RESUMED and REPLAYED from a guess.
//   members   stable counting sort of (label, point id) -> per-cell member lists in ascending point order; for clouds of at most 32 768
//             points made inside the model kernel instead (every cell's workgroup lists its own members, round 5)
//   centres   sequential fp32 sum in member order: bit for bit the reference's cell means (inside the model kernel since round 5)
//   model     a workgroup of four groups of 128 lanes per cell, one lane per monomial: the groups take the member tiles in turn, fp32
//             accumulation per group in member order, the groups' sums added in group order
//   predict   one lane per query, cells broadcast from SGPRs, the polynomial evaluated by a nested Horner scheme whose
//             coefficients stream through scalar loads in traversal order (no per-lane monomial table)
//
// Everything is deterministic (no float atomics).  Differences from cpu-slam come from expf (1 ulp) and the Horner
// evaluation order only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "cpd_fgt.h"
#include "cpd_kernels.h"
#include "reduce.hpp"

namespace mislam {

__device__ __forceinline__ float len2(float x, float y, float z) { return (x * x + y * y) + z * z; }   // point.h:49-51

// ---------------------------------------------------------------------------------------------------------------
// KCenter (fgt.cpp:152-193)
// ---------------------------------------------------------------------------------------------------------------
struct ArgMax {
    float v;
    int i;
    float x, y, z;
};

static_assert(sizeof(ArgMax) == 20 && FGT_SWEEP_SCRATCH_BYTES >= (FGT_GRID_SWEEP_BLOCKS + 1) * sizeof(ArgMax), "sweep scratch size");

__device__ __forceinline__ bool beats(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }

__device__ __forceinline__ ArgMax wave_argmax(ArgMax a)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        ArgMax o;
        o.v = __shfl_down(a.v, off, 64);
        o.i = __shfl_down(a.i, off, 64);
        o.x = __shfl_down(a.x, off, 64);
        o.y = __shfl_down(a.y, off, 64);
        o.z = __shfl_down(a.z, off, 64);
        if (beats(o.v, o.i, a.v, a.i)) a = o;
    }
    return a;
}

// (distance, index) as ONE unsigned key that orders like beats(): a distance >= +0 orders like its bits, and among equal distances the
// LOWER index must win a maximum -- so the index goes in complemented.  0 = no candidate (v < 0).
__device__ __forceinline__ unsigned long long argmax_key(float v, int i)
{
    return v < 0.f ? 0ull : (((unsigned long long)__float_as_uint(v) << 32) | (unsigned long long)(0xffffffffu - (unsigned int)i));
}
__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long k, int width)      // maximum over aligned groups of `width` lanes
{
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        if (off >= width) break;
        const unsigned int lo = (unsigned int)__shfl_xor((int)(unsigned int)k, off, 64), hi = (unsigned int)__shfl_xor((int)(unsigned int)(k >> 32), off, 64);
        const unsigned long long o = ((unsigned long long)hi << 32) | lo;
        k = o > k ? o : k;
    }
    return k;
}

// PER > 0: every lane keeps its PER points (id = lane + r * 1024), their distances and labels in registers.
// PER == 0: any n; distances and labels stay in global memory (each lane only ever touches its own entries).
// The sweep is prefix-stable (the first k centres do not depend on K), so a finished sweep can be RESUMED: with start > 0 the
// kernel picks up the distances and labels steps 0..start-1 left in dist/indx and runs steps start..K-1 only.  The fixed cloud
// of a CPD run is clustered this way: K grows as sigma^2 shrinks, and each new E-step only adds the missing centres.
// `picked[k]` receives the id of centre k (the sweep's own record of what it chose: next E-step's guess, see fgt_replay_kernel);
// start_ptr != null: the number of finished steps is read from the device (what a replay verified) instead of `start`.
template <int PER>
__global__ __launch_bounds__(1024) void fgt_kcenter_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                           const float* __restrict__ z, int n, int start, const int* __restrict__ start_ptr, int K,
                                                           float* __restrict__ dist, int* __restrict__ indx, int* __restrict__ picked)
{
    if (start_ptr != nullptr) start = *start_ptr;
    if (start >= K) return;                         // (a replay that covered every step: dist / indx are final)
    // per wave: its best key and that point's coordinates.  Double-buffered: a wave can run at most one barrier ahead of the slowest reader
    __shared__ unsigned long long s_key[2][16];
    __shared__ float4 s_xyz[2][16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr int NR = PER > 0 ? PER : 1;
    float px[NR], py[NR], pz[NR], pd[NR];
    int pc[NR];
    ArgMax best = {-1.f, 0x7fffffff, 0.f, 0.f, 0.f};
    if (PER > 0) {
#pragma unroll
        for (int r = 0; r < NR; r++) {
            const int j = tid + r * 1024, jc = min(j, n - 1);
            px[r] = x[jc]; py[r] = y[jc]; pz[r] = z[jc];
            // a point's distance to its nearest centre so far: +inf before the first centre (step 0 then takes every distance as it
            // comes), -inf for the register slots past the cloud's end (never closer to anything, never a maximum) -- so that the
            // sweep below needs no branch and no special first step
            pd[r] = j < n ? __builtin_inff() : -__builtin_inff(); pc[r] = 0;
            if (start > 0) {
                if (j < n) { pd[r] = dist[jc]; pc[r] = indx[jc]; }
                if (j < n && pd[r] > best.v) best = {pd[r], j, px[r], py[r], pz[r]};
            }
        }
    } else if (start > 0) {
        for (int j = tid; j < n; j += 1024) {
            const float cur = dist[j];
            if (cur > best.v) best = {cur, j, x[j], y[j], z[j]};
        }
    }
    float cx = x[1], cy = y[1], cz = z[1];          // the first centre is point 1 (fgt.cpp:162)
    for (int step = start; step < K; step++) {
        if (step > 0) {
            // this step's centre = FIRST maximum of the distance array (std::max_element, fgt.cpp:179): the maximum of the keys -- over the
            // wave (12 exchanges of one word, where the five-field record took 30), whose holder alone writes its coordinates; then over
            // the 16 waves, one key per lane of a group of 16 (8 exchanges and two LDS reads, where every lane read all 16 records)
            const int buf = step & 1;
            const unsigned long long mine = argmax_key(best.v, best.i);
            const unsigned long long wmax = wave_max_u64(mine, 64);
            if (wmax == 0ull ? lane == 0 : mine == wmax) {            // (keys of distinct points differ; no candidate at all: lane 0 says so)
                s_key[buf][wave] = wmax;
                s_xyz[buf][wave] = make_float4(best.x, best.y, best.z, 0.f);
            }
            __syncthreads();
            const unsigned long long kq = s_key[buf][lane & 15];
            const unsigned long long kmax = wave_max_u64(kq, 16);
            const int q = __builtin_ctzll(__builtin_amdgcn_ballot_w64(kq == kmax));      // (a lane of the first group of 16: q = its wave number)
            const float4 w = s_xyz[buf][q & 15];
            cx = w.x; cy = w.y; cz = w.z;
            if (tid == 0) picked[step] = (int)(0xffffffffu - (unsigned int)kmax);
        } else if (tid == 0) picked[0] = 1;
        best = {-1.f, 0x7fffffff, 0.f, 0.f, 0.f};
        if (PER > 0) {
#pragma unroll
            for (int r = 0; r < NR; r++) {
                const int j = tid + r * 1024;
                const float d = len2(px[r] - cx, py[r] - cy, pz[r] - cz);
                const bool closer = d < pd[r];                           // strict <: fgt.cpp:187 (always at step 0, never for a slot past the end)
                const float cur = closer ? d : pd[r];
                pc[r] = closer ? step : pc[r];
                pd[r] = cur;
                const bool further = cur > best.v;                       // ascending j per lane: the first maximum stays
                best.v = further ? cur : best.v; best.i = further ? j : best.i;
                best.x = further ? px[r] : best.x; best.y = further ? py[r] : best.y; best.z = further ? pz[r] : best.z;
            }
        } else {
            for (int j = tid; j < n; j += 1024) {
                const float qx = x[j], qy = y[j], qz = z[j];
                const float d = len2(qx - cx, qy - cy, qz - cz);
                float cur;
                if (step == 0) { cur = d; dist[j] = d; indx[j] = 0; }
                else {
                    cur = dist[j];
                    if (d < cur) { cur = d; dist[j] = d; indx[j] = step; }
                }
                if (cur > best.v) best = {cur, j, qx, qy, qz};
            }
        }
    }
    if (PER > 0) {
#pragma unroll
        for (int r = 0; r < NR; r++) {
            const int j = tid + r * 1024;
            if (j < n) { indx[j] = pc[r]; dist[j] = pd[r]; }
        }
    }
}

// The same sweep on SEVERAL workgroups in ONE launch (round 5; clouds beyond the 16 384 points one workgroup holds in registers, up to
// FGT_COOP_MAX_POINTS): workgroup g keeps points [g * 1024 * PER, (g + 1) * 1024 * PER) in registers exactly as the kernel above keeps the whole
// cloud, and a step's arg-max goes through memory: every workgroup posts its best (key, coordinates) into this step's slot, takes a ticket
// behind an agent-scope release, waits for the tickets of all G workgroups, and reads the G slots back -- one wave, one slot per lane (G <= 64).
// Slots are double-buffered by the step's parity (a workgroup can be at most one barrier ahead of the slowest reader); the ticket counter only
// grows (zeroed by the host before the launch).  The keys are the one-workgroup kernel's (distance bits, complemented index): the same first
// maximum, the same centres, the same labels, bit for bit.  Launched COOPERATIVELY (all G workgroups resident, or the launch fails and the
// caller falls back): the wait below ends because every workgroup reaches every barrier -- `start` and K are the same for all of them.
struct CoopSlot {
    unsigned long long key;
    float x, y, z, pad;
};
static_assert(sizeof(CoopSlot) == 24 || sizeof(CoopSlot) == 32, "slot layout");
constexpr int FGT_COOP_MAX_GROUPS = 64;
constexpr int FGT_COOP_MIN_STEPS = 16;             // (MISLAM_FGT_COOP_SWEEP=2: every sweep, whatever its length -- tests)
constexpr int FGT_COOP_MAX_POINTS = FGT_COOP_MAX_GROUPS * 1024 * 16;
static_assert(FGT_SWEEP_SCRATCH_BYTES >= 64 + 2 * FGT_COOP_MAX_GROUPS * sizeof(CoopSlot), "the cooperative sweep's counter and slots fit the sweep scratch");
template <int PER>
__global__ __launch_bounds__(1024) void fgt_kcenter_coop_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ z, int n,
                                                                int start, const int* __restrict__ start_ptr, int K, float* __restrict__ dist,
                                                                int* __restrict__ indx, int* __restrict__ picked, unsigned int* counter, CoopSlot* slots)
{
    if (start_ptr != nullptr) start = *start_ptr;
    if (start >= K) return;                         // (the same for every workgroup: nobody waits for anybody)
    __shared__ unsigned long long s_key[16];
    __shared__ float4 s_xyz[16];
    __shared__ float4 s_centre;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, G = (int)gridDim.x;
    const int base = (int)blockIdx.x * 1024 * PER;
    float px[PER], py[PER], pz[PER], pd[PER];
    int pc[PER];
    ArgMax best = {-1.f, 0x7fffffff, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < PER; r++) {
        const int j = base + tid + r * 1024, jc = min(j, n - 1);
        px[r] = x[jc]; py[r] = y[jc]; pz[r] = z[jc];
        pd[r] = j < n ? __builtin_inff() : -__builtin_inff(); pc[r] = 0;      // as in fgt_kcenter_kernel
        if (start > 0) {
            if (j < n) { pd[r] = dist[jc]; pc[r] = indx[jc]; }
            if (j < n && pd[r] > best.v) best = {pd[r], j, px[r], py[r], pz[r]};
        }
    }
    float cx = x[1], cy = y[1], cz = z[1];          // the first centre is point 1 (fgt.cpp:162)
    unsigned int barriers = 0u;
    for (int step = start; step < K; step++) {
        if (step > 0) {
            const unsigned long long mine = argmax_key(best.v, best.i);
            const unsigned long long wmax = wave_max_u64(mine, 64);
            if (wmax == 0ull ? lane == 0 : mine == wmax) {
                s_key[wave] = wmax;
                s_xyz[wave] = make_float4(best.x, best.y, best.z, 0.f);
            }
            __syncthreads();
            if (wave == 0) {
                const unsigned long long kq = s_key[lane & 15];
                const unsigned long long kmax = wave_max_u64(kq, 16);
                const int q = __builtin_ctzll(__builtin_amdgcn_ballot_w64(kq == kmax)) & 15;
                CoopSlot* row = slots + (size_t)(step & 1) * FGT_COOP_MAX_GROUPS;
                barriers += 1u;
                if (lane == 0) {
                    const float4 w = s_xyz[q];
                    CoopSlot* mine_slot = row + blockIdx.x;
                    mine_slot->key = kmax; mine_slot->x = w.x; mine_slot->y = w.y; mine_slot->z = w.z;
                    __threadfence();                                   // release: the slot before the ticket
                    atomicAdd(counter, 1u);
                    const unsigned int target = barriers * (unsigned int)G;
                    while (__hip_atomic_load(counter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) __builtin_amdgcn_s_sleep(1);
                    __threadfence();                                   // acquire: the other workgroups' slots
                }
                // (the same wave, behind lane 0's fences in program order)
                unsigned long long ok = 0ull;
                float ox = 0.f, oy = 0.f, oz = 0.f;
                if (lane < G) {
                    const CoopSlot* o = row + lane;
                    ok = __hip_atomic_load(&o->key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    ox = __hip_atomic_load(&o->x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    oy = __hip_atomic_load(&o->y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    oz = __hip_atomic_load(&o->z, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
                const unsigned long long gmax = wave_max_u64(ok, 64);
                const int winner = __builtin_ctzll(__builtin_amdgcn_ballot_w64(ok == gmax));   // (keys of distinct points differ; all zero: lane 0, as there)
                const float wx = __shfl(ox, winner, 64), wy = __shfl(oy, winner, 64), wz = __shfl(oz, winner, 64);
                if (lane == 0) {
                    s_centre = make_float4(wx, wy, wz, 0.f);
                    if (blockIdx.x == 0) picked[step] = (int)(0xffffffffu - (unsigned int)gmax);
                }
            }
            __syncthreads();
            cx = s_centre.x; cy = s_centre.y; cz = s_centre.z;
        } else if (blockIdx.x == 0 && tid == 0) picked[0] = 1;
        best = {-1.f, 0x7fffffff, 0.f, 0.f, 0.f};
#pragma unroll
        for (int r = 0; r < PER; r++) {
            const int j = base + tid + r * 1024;
            const float d = len2(px[r] - cx, py[r] - cy, pz[r] - cz);
            const bool closer = d < pd[r];                               // strict <: fgt.cpp:187
            const float cur = closer ? d : pd[r];
            pc[r] = closer ? step : pc[r];
            pd[r] = cur;
            const bool further = cur > best.v;                           // ascending j per lane: the first maximum stays
            best.v = further ? cur : best.v; best.i = further ? j : best.i;
            best.x = further ? px[r] : best.x; best.y = further ? py[r] : best.y; best.z = further ? pz[r] : best.z;
        }
    }
#pragma unroll
    for (int r = 0; r < PER; r++) {
        const int j = base + tid + r * 1024;
        if (j < n) { indx[j] = pc[r]; dist[j] = pd[r]; }
    }
}

// The same sweep for large clouds, one step per launch over the whole grid.  step_kernel applies centre `cur` (step 0: point 1)
// to every point -- or, scan_only, just reads the distances a finished sweep left -- and posts each workgroup's arg-max (first
// maximum: every lane walks ascending indices, ties go to the lower index); pick_kernel reduces those to the next centre.
__global__ __launch_bounds__(256) void fgt_sweep_step_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                             const float* __restrict__ z, int n, const ArgMax* __restrict__ cur, int step,
                                                             int scan_only, float* __restrict__ dist, int* __restrict__ indx,
                                                             ArgMax* __restrict__ partials, int* __restrict__ picked)
{
    if (step == 0 && !scan_only && blockIdx.x == 0 && threadIdx.x == 0) picked[0] = 1;
    __shared__ ArgMax s_best[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float cx, cy, cz;
    if (step == 0) { cx = x[1]; cy = y[1]; cz = z[1]; }     // fgt.cpp:162
    else { cx = cur->x; cy = cur->y; cz = cur->z; }
    ArgMax best = {-1.f, 0x7fffffff, 0.f, 0.f, 0.f};
    for (int j = blockIdx.x * 256 + tid; j < n; j += gridDim.x * 256) {
        const float qx = x[j], qy = y[j], qz = z[j];
        float v;
        if (scan_only) v = dist[j];
        else {
            const float d = len2(qx - cx, qy - cy, qz - cz);
            if (step == 0) { v = d; dist[j] = d; indx[j] = 0; }
            else {
                v = dist[j];
                if (d < v) { v = d; dist[j] = d; indx[j] = step; }       // strict <: fgt.cpp:187
            }
        }
        if (v > best.v) best = {v, j, qx, qy, qz};
    }
    best = wave_argmax(best);
    if (lane == 0) s_best[wave] = best;
    __syncthreads();
    if (tid == 0) {
        ArgMax w = s_best[0];
        for (int q = 1; q < 4; q++) if (beats(s_best[q].v, s_best[q].i, w.v, w.i)) w = s_best[q];
        partials[blockIdx.x] = w;
    }
}

__global__ __launch_bounds__(256) void fgt_sweep_pick_kernel(const ArgMax* __restrict__ partials, int count, ArgMax* __restrict__ cur,
                                                             int* __restrict__ picked_slot)
{
    __shared__ ArgMax s_best[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    ArgMax best = {-1.f, 0x7fffffff, 0.f, 0.f, 0.f};
    for (int q = tid; q < count; q += 256) {
        const ArgMax o = partials[q];
        if (beats(o.v, o.i, best.v, best.i)) best = o;
    }
    best = wave_argmax(best);
    if (lane == 0) s_best[wave] = best;
    __syncthreads();
    if (tid == 0) {
        ArgMax w = s_best[0];
        for (int q = 1; q < 4; q++) if (beats(s_best[q].v, s_best[q].i, w.v, w.i)) w = s_best[q];
        *cur = w;
        *picked_slot = w.i;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// The sweep REPLAYED.  The farthest-point sweep is a chain -- centre k is the arg-max of the distances centres 0..k-1 leave -- and
// on one workgroup it costs ~1.2 us per step; but CPD clusters the moving cloud again every E-step, and between two E-steps that
// cloud only undergoes a similarity transform: the sweep picks the same points in the same order unless rounding flips a near-tie.
// So the previous E-step's picks are a GUESS, and a guess can be checked without a chain: with the centres known, every point's
// running minimum over them is independent of every other point (one lane per point, the centres broadcast from LDS), and "the
// arg-max before centre i is applied is the guessed point i" is one reduction per step.  replay<ARGMAX = true> does both in one
// pass over the whole chip and posts each wave's arg-max per step; check reduces those over the waves and leaves in state[0] the
// first step the guess fails at (or the guess's length).  If it failed, a second replay<false> restores distances and labels after
// only the verified steps (it exits at once if all held); the chain kernel then resumes from state[0].  Distances, labels and
// the tie rules are the chain's own arithmetic: the result is the chain's, bit for bit, whatever the guess was.
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float wave_max_f32(float v)
{
    // quads (xor 1, xor 2), halves of a row (row_half_mirror), rows of 16 (row_mirror): maxima are idempotent, mirrors do
    v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xf, 0xf, true)));
    v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xf, 0xf, true)));
    v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x141, 0xf, 0xf, true)));
    v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x140, 0xf, 0xf, true)));
    const float r0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0)), r1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 16)),
                r2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 32)), r3 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 48));
    return fmaxf(fmaxf(r0, r1), fmaxf(r2, r3));
}

// One wave per workgroup, P points per lane: id = (workgroup * P + r) * 64 + lane.  limit_ptr != null (the second pass): the number of
// centres is read from the device, and the launch has nothing to do if it is skip_if_ge or more.
template <int P, bool ARGMAX>
__global__ __launch_bounds__(64) void fgt_replay_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ z, int n,
                                                        const int* __restrict__ picked, int limit, const int* __restrict__ limit_ptr, int skip_if_ge,
                                                        float* __restrict__ dist, int* __restrict__ indx, unsigned long long* __restrict__ partial,
                                                        int* __restrict__ state)
{
    extern __shared__ float4 s_centre[];
    int lim = limit;
    if (limit_ptr != nullptr) { lim = *limit_ptr; if (lim >= skip_if_ge) return; }
    const int lane = (int)threadIdx.x;
    if (ARGMAX && blockIdx.x == 0 && lane == 0) state[0] = lim;          // no step disproved yet (the check kernel lowers it)
    for (int i = lane; i < lim; i += 64) { const int j = picked[i]; s_centre[i] = make_float4(x[j], y[j], z[j], 0.f); }
    __syncthreads();
    float px[P], py[P], pz[P], pd[P];
    int pc[P];
#pragma unroll
    for (int r = 0; r < P; r++) {
        const int j = ((int)blockIdx.x * P + r) * 64 + lane, jc = min(j, n - 1);
        px[r] = x[jc]; py[r] = y[jc]; pz[r] = z[jc];
        pd[r] = j < n ? __builtin_inff() : -__builtin_inff(); pc[r] = 0;      // as in fgt_kcenter_kernel
    }
    const size_t W = gridDim.x;
    for (int i = 0; i < lim; i++) {
        if (ARGMAX && i > 0) {
            // what the sweep picks as centre i: the FIRST maximum of the distances as centres 0..i-1 leave them (fgt.cpp:179)
            float bv = pd[0];
            int br = 0;
#pragma unroll
            for (int r = 1; r < P; r++) { const bool further = pd[r] > bv; bv = further ? pd[r] : bv; br = further ? r : br; }   // ascending ids per lane
            const float wv = wave_max_f32(bv);
            unsigned long long tied = __builtin_amdgcn_ballot_w64(bv == wv);
            int first;
            if (P == 1) first = (int)blockIdx.x * 64 + __builtin_ctzll(tied);          // ids ascend with the lane
            else {
                const int id = ((int)blockIdx.x * P + br) * 64 + lane;
                first = 0x7fffffff;
                while (tied != 0ull) { first = min(first, __builtin_amdgcn_readlane(id, __builtin_ctzll(tied))); tied &= tied - 1ull; }
            }
            if (lane == 0) partial[(size_t)i * W + blockIdx.x] = argmax_key(wv, first);
        }
        const float4 c = s_centre[i];
#pragma unroll
        for (int r = 0; r < P; r++) {
            const float d = len2(px[r] - c.x, py[r] - c.y, pz[r] - c.z);
            const bool closer = d < pd[r];                               // strict <: fgt.cpp:187
            pc[r] = closer ? i : pc[r];
            pd[r] = closer ? d : pd[r];
        }
    }
#pragma unroll
    for (int r = 0; r < P; r++) {
        const int j = ((int)blockIdx.x * P + r) * 64 + lane;
        if (j < n) { indx[j] = pc[r]; dist[j] = pd[r]; }
    }
}

// one wave per step i in [1, lim): the maximum of the W keys posted for it names the point the sweep picks as centre i
__global__ __launch_bounds__(256) void fgt_replay_check_kernel(const unsigned long long* __restrict__ partial, int W, const int* __restrict__ picked,
                                                               int lim, int* __restrict__ state)
{
    const int lane = (int)threadIdx.x & 63, i = 1 + (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
    if (blockIdx.x == 0 && threadIdx.x == 0 && picked[0] != 1) atomicMin(&state[0], 0);      // centre 0 is point 1 (fgt.cpp:162)
    if (i >= lim) return;
    unsigned long long k = 0ull;
    for (int q = lane; q < W; q += 64) { const unsigned long long o = partial[(size_t)i * (size_t)W + q]; k = o > k ? o : k; }
    k = wave_max_u64(k, 64);
    if (lane == 0 && (k == 0ull || (int)(0xffffffffu - (unsigned int)k) != picked[i])) atomicMin(&state[0], i);
}

// ---------------------------------------------------------------------------------------------------------------
// member lists: memb = point ids grouped by cluster, ASCENDING inside a cluster (the order fgt.cpp:195-210 sums the cell means
// in), off[k] = start of cluster k.  A stable counting sort on the labels, in three small launches and no library call:
// the cloud is cut into G chunks of consecutive ids, one wave each; (1) per-chunk label counts H[g][k]; (2) per label, the
// exclusive prefix of the counts over the chunks, and the cluster starts off[k]; (3) every wave places its chunk, 64 points per
// step in id order: the lanes holding the same label are found with ballots, ranked by lane, and take the next slots of that
// label's run -- the chunk-private cursor H[g][k] is advanced by one atomic per distinct label and step.
// ---------------------------------------------------------------------------------------------------------------
constexpr int FGT_LIST_LDS_LABELS = 8192;   // up to this many labels a chunk's cursors live in LDS (32 KB per wave)

// lanes of the wave that hold the same label as this one (valid lanes only): one ballot per label BIT instead of one round per
// distinct label -- a chunk's 64 labels are mostly distinct, and the rounds were 64 dependent readlane / ballot / atomic steps
__device__ __forceinline__ unsigned long long same_label_lanes(int lab, bool valid, int label_bits)
{
    unsigned long long same = __builtin_amdgcn_ballot_w64(valid);
    for (int b = 0; b < label_bits; b++) {
        const bool bit = ((lab >> b) & 1) != 0;
        const unsigned long long with = __builtin_amdgcn_ballot_w64(bit);
        same &= bit ? with : ~with;
    }
    return same;
}

// SCATTER == false: H[g][k] = how many points of chunk g carry label k.  SCATTER == true: H[g][k] holds the number of label-k points in the
// chunks before g (fgt_lists_columns_kernel); every point goes to memb[off[k] + that + its rank among the chunk's label-k points].
// K <= FGT_LIST_LDS_LABELS: the chunk's row lives in LDS (count: zeroed there and written out whole, no memset, no global atomics).
// SCAN_OFF (K <= FGT_LIST_SCAN_LABELS): off[] is not read but computed here, from tot[] (an exclusive prefix sum per wave, K / 64 steps)
// into LDS -- workgroup 0 also writes it out for the kernels that follow; saves the one-workgroup offsets launch in between.
constexpr int FGT_LIST_SCAN_LABELS = 1024;
template <bool SCATTER, bool SCAN_OFF>
__global__ __launch_bounds__(64) void fgt_lists_pass_kernel(const int* __restrict__ indx, int n, int K, int chunk, int label_bits, int* __restrict__ H,
                                                            const int* __restrict__ tot, int* __restrict__ off, int* __restrict__ memb)
{
    extern __shared__ int cur[];                                 // K <= FGT_LIST_LDS_LABELS: this chunk's counter / cursor per label [+ K + 1 offsets]
    const int lane = threadIdx.x;
    const int lo = blockIdx.x * chunk, hi = lo + chunk < n ? lo + chunk : n;
    int* __restrict__ row = H + (size_t)blockIdx.x * K;
    const bool lds = K <= FGT_LIST_LDS_LABELS;
    int* s_off = cur + K;
    if (lds)
        for (int k = lane; k < K; k += 64) cur[k] = SCATTER ? row[k] : 0;      // one wave: LDS operations of a wave complete in order
    if (SCATTER && SCAN_OFF) {
        int carry = 0;
        for (int k0 = 0; k0 < K; k0 += 64) {
            const int k = k0 + lane;
            const int c = k < K ? tot[k] : 0;
            int incl = c;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int t = __shfl_up(incl, o, 64);
                if (lane >= o) incl += t;
            }
            if (k < K) { s_off[k] = carry + incl - c; if (blockIdx.x == 0) off[k] = carry + incl - c; }
            carry += __shfl(incl, 63, 64);
        }
        if (blockIdx.x == 0 && lane == 0) off[K] = carry;
    }
    for (int i0 = lo; i0 < hi; i0 += 64) {
        const int i = i0 + lane;
        const bool valid = i < hi;
        const int lab = valid ? indx[i] : -1;
        const unsigned long long same = same_label_lanes(lab, valid, label_bits);
        const int cnt = (int)__builtin_popcountll(same);
        const int rank = (int)__builtin_popcountll(same & ((1ull << lane) - 1ull));
        const bool leader = valid && rank == 0;                  // (the leaders of a step hold distinct labels)
        if (!SCATTER) {
            if (leader) { if (lds) cur[lab] += cnt; else atomicAdd(&row[lab], cnt); }
        } else {
            int before = 0;
            if (leader) {
                if (lds) { before = cur[lab]; cur[lab] = before + cnt; }
                else before = atomicAdd(&row[lab], cnt);         // very many labels: the wave's own cursor in memory (uncontended, L2-coherent)
            }
            before = __shfl(before, valid ? __builtin_ctzll(same) : lane, 64);
            if (valid) memb[(SCAN_OFF ? s_off[lab] : off[lab]) + before + rank] = i;
        }
    }
    if (!SCATTER && lds)
        for (int k = lane; k < K; k += 64) row[k] = cur[k];
}

// per label: H[g][k] <- sum of the counts of the chunks before g; tot[k] <- the label's total.  One wave per label, 64 chunks per
// step (a wave-wide exclusive scan), the carry in a scalar.
__global__ __launch_bounds__(256) void fgt_lists_columns_kernel(int* __restrict__ H, int G, int K, int* __restrict__ tot)
{
    const int k = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (k >= K) return;
    int carry = 0;
    for (int g0 = 0; g0 < G; g0 += 64) {
        const int g = g0 + lane;
        const int c = g < G ? H[(size_t)g * K + k] : 0;
        int incl = c;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(incl, o, 64);
            if (lane >= o) incl += t;
        }
        if (g < G) H[(size_t)g * K + k] = carry + incl - c;
        carry += __shfl(incl, 63, 64);
    }
    if (lane == 0) tot[k] = carry;
}

// off[0..K] <- exclusive prefix of tot[0..K) (one workgroup)
__global__ __launch_bounds__(1024) void fgt_lists_offsets_kernel(const int* __restrict__ tot, int K, int* __restrict__ off)
{
    __shared__ int s[1024];
    __shared__ int carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int base = 0; base < K; base += 1024) {
        const int k = base + (int)threadIdx.x;
        const int v = k < K ? tot[k] : 0;
        s[threadIdx.x] = v;
        __syncthreads();
        for (int o = 1; o < 1024; o <<= 1) {
            const int t = (int)threadIdx.x >= o ? s[threadIdx.x - o] : 0;
            __syncthreads();
            s[threadIdx.x] += t;
            __syncthreads();
        }
        if (k < K) off[k] = carry + s[threadIdx.x] - v;
        __syncthreads();
        if (threadIdx.x == 1023) carry += s[1023];
        __syncthreads();
    }
    if (threadIdx.x == 0) off[K] = carry;
}

constexpr int FGT_TILE = 128;   // members staged through LDS per step of the centre / model kernels (= their block size)

// Cell means: sequential fp32 sums in ascending point order, then * (1.0f / count)   (fgt.cpp:195-210).  One workgroup per
// cell: the members' coordinates are gathered 128 at a time (coalesced index reads, one gather per lane) into LDS, and lanes
// 0..2 run the three serial sums out of LDS -- the chain of dependent adds is the only serial part left.
__global__ __launch_bounds__(FGT_TILE) void fgt_centers_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                               const float* __restrict__ z, const int* __restrict__ memb,
                                                               const int* __restrict__ off, int K, float* __restrict__ xc)
{
    __shared__ float s[3][FGT_TILE];
    const int k = blockIdx.x, tid = threadIdx.x;
    const int j0 = off[k], j1 = off[k + 1];
    float sum = 0.f;
    for (int base = j0; base < j1; base += FGT_TILE) {
        const int cnt = min(FGT_TILE, j1 - base);
        if (tid < cnt) {
            const int i = memb[base + tid];
            s[0][tid] = x[i]; s[1][tid] = y[i]; s[2][tid] = z[i];
        }
        __syncthreads();
        if (tid < 3) {
#pragma unroll 8
            for (int q = 0; q < cnt; q++) sum += s[tid][q];
        }
        __syncthreads();
    }
    // an empty cell gives 0 * inf = NaN, exactly as the reference
    if (tid < 3) xc[3 * k + tid] = sum * (1.0f / (float)(j1 - j0));
    (void)K;
}

// ---------------------------------------------------------------------------------------------------------------
// ComputeA_k (fgt.cpp:246-302): workgroup = one cell, lane t = one monomial, accumulated over the members of the cell in the
// reference's order.  Per tile of 128 members each lane prepares ONE member (powers of its scaled offset, exp(-|dx|^2),
// weights) in LDS; all lanes then walk the tile: three power look-ups, three multiplies and W multiply-adds per member.
// ---------------------------------------------------------------------------------------------------------------
// Round 5: FGT_MODEL_GROUPS groups of 128 threads per workgroup.  A cell has 130 - 550 members on the bunny clouds and there are only 51 - 117 cells:
// with one group (rounds 1 - 4) a workgroup walked its members tile after tile on two waves while most of the chip idled -- 24 - 30 us per launch.
// Group g now takes the tiles g, g + G, ... of the cell (prepares and walks them on its own LDS arrays), and the groups' sums are added in group
// order at the end: ((g0 + g1) + g2) + g3 -- a fixed order (bitwise reproducible); against the reference's one-by-one order the last bits move, as
// they do in every fp32 sum of this E-step (FGT arrays agree with the reference's to 1e-5 of the largest entry, tests/test_gpu_fgt.py).  A cell of
// at most 128 members is group 0's alone: the same bits as before.
constexpr int FGT_MODEL_GROUPS = 4;
// LISTS (round 5, clouds of at most FGT_LISTS_IN_MODEL_MAX_POINTS points): the cell's member list is made HERE, by the workgroup that is about to walk it --
// fgt_lists_pass_kernel's stable counting sort seen from one cell: the list starts behind every point with a smaller label (off[k]) and holds the
// points labelled k in ascending order.  Two passes over the labels (a few tens of KB, in the caches), each wave a contiguous range: count, then place
// by a ballot prefix.  The same off / memb as the three sort launches leave (every workgroup of the cell writes the same words), without the launches.
constexpr int FGT_LISTS_IN_MODEL_MAX_POINTS = 32768;
constexpr long long FGT_LISTS_IN_MODEL_MAX_READS = 4ll << 20;    // K workgroups read n labels each: beyond this the counting sort's O(n) wins (bunny: K <= 281)
// the size rule alone (n and K: what the host needs to keep the build's PATH a function of the problem, not of which E-step it is)
bool fgt_lists_rule(int n, int K)
{
    return n <= FGT_LISTS_IN_MODEL_MAX_POINTS && (long long)K * n <= FGT_LISTS_IN_MODEL_MAX_READS;
}
static bool lists_in_model(const FgtClusters& c)
{
    return c.lists_in_model && c.centers_in_model && fgt_lists_rule(c.n, c.K);
}
template <int W, bool CENTERS, bool LISTS>
__global__ __launch_bounds__(FGT_TILE * FGT_MODEL_GROUPS) void fgt_model_kernel(FgtClusters c, const float4* __restrict__ w4, float inv_sigma, FgtTables t,
                                                                                float* __restrict__ B)
{
    constexpr int G = FGT_MODEL_GROUPS;
    static_assert(!LISTS || CENTERS, "a clustering that leaves its lists to the model build leaves its means too");
    // powers d^0..d^(p-1) of the three scaled offsets of every member of the tile; rows padded by one word so that lanes
    // reading different powers of the same member fall into different LDS banks
    __shared__ float sp[G][3][FGT_MAX_ORDER][FGT_TILE + 1];
    __shared__ float se[G][FGT_TILE];
    __shared__ float sw[G][W][FGT_TILE];
    const int k = blockIdx.x, tid = threadIdx.x & (FGT_TILE - 1), grp = threadIdx.x / FGT_TILE;
    const int m = blockIdx.y * FGT_TILE + tid;
    const bool live = m < t.pd;
    const unsigned int e = t.mono[live ? m : 0];
    const int ea = e & 0xff, eb = (e >> 8) & 0xff, ec = (e >> 16) & 0xff;
    int j0, j1;
    if (LISTS) {
        constexpr int NW = FGT_TILE * G / 64;
        __shared__ int s_lt[NW], s_eq[NW];
        const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
        const int per = ((c.n + NW * 64 - 1) / (NW * 64)) * 64;          // the wave's range of points, whole steps of 64
        const int r0 = min(c.n, wave * per), r1 = min(c.n, r0 + per);
        // pass 1: the labels of the wave's range, at most 64 steps (32 768 points over eight waves); what a lane needs of them for pass 2 is one bit
        // per step -- kept, so that the second pass is stores only (loads behind stores to memory the compiler cannot tell apart would each wait)
        static_assert(FGT_LISTS_IN_MODEL_MAX_POINTS <= NW * 64 * 64, "a lane's steps fit one 64-bit mask");
        const int* __restrict__ labels = c.indx;
        int lt = 0, eq = 0;
        unsigned long long mine_bits = 0ull;
        const int steps = (r1 - r0 + 63) / 64;
        for (int s0 = 0; s0 < steps; s0 += 16) {                        // sixteen steps' labels in flight
            int lab[16];
#pragma unroll
            for (int j = 0; j < 16; j++) {
                const int i = r0 + (s0 + j) * 64 + lane;
                lab[j] = i < r1 ? labels[i] : 0x7fffffff;
            }
#pragma unroll
            for (int j = 0; j < 16; j++) {
                lt += __builtin_popcountll(__builtin_amdgcn_ballot_w64(lab[j] < k));
                eq += __builtin_popcountll(__builtin_amdgcn_ballot_w64(lab[j] == k));
                mine_bits |= (unsigned long long)(lab[j] == k) << (s0 + j);
            }
        }
        if (lane == 0) { s_lt[wave] = lt; s_eq[wave] = eq; }
        __syncthreads();
        int first = 0, count = 0, before = 0;
#pragma unroll
        for (int w2 = 0; w2 < NW; w2++) {
            first += s_lt[w2];
            before += w2 < wave ? s_eq[w2] : 0;
            count += s_eq[w2];
        }
        int at = first + before;
        for (int step = 0; step < steps; step++) {
            const bool mine = ((mine_bits >> step) & 1ull) != 0ull;
            const unsigned long long mk = __builtin_amdgcn_ballot_w64(mine);
            if (mk == 0ull) continue;
            if (mine) c.memb[at + (int)__builtin_amdgcn_mbcnt_hi((unsigned int)(mk >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)mk, 0u))] = r0 + step * 64 + lane;
            at += __builtin_popcountll(mk);
        }
        if (threadIdx.x == 0) {
            c.off[k] = first;
            if (k == c.K - 1) c.off[c.K] = first + count;
        }
        __syncthreads();                                               // (the list is this workgroup's own writes: one CU, one L1)
        j0 = first; j1 = first + count;
    } else {
        j0 = c.off[k]; j1 = c.off[k + 1];
    }
    float cx, cy, cz;
    if (CENTERS) {
        // the cell's mean first -- fgt_centers_kernel's arithmetic (sequential fp32 sums in ascending point order, * (1.0f / count): fgt.cpp:195-210),
        // here instead of in a launch of its own; every workgroup of the cell computes it, the first one leaves it in xc for the transform
        __shared__ float sc[3][FGT_TILE * G];
        __shared__ float mean[3];
        float sum = 0.f;
        for (int base = j0; base < j1; base += FGT_TILE * G) {
            const int cnt = min(FGT_TILE * G, j1 - base);
            if ((int)threadIdx.x < cnt) {
                const int i = c.memb[base + threadIdx.x];
                sc[0][threadIdx.x] = c.x[i]; sc[1][threadIdx.x] = c.y[i]; sc[2][threadIdx.x] = c.z[i];
            }
            __syncthreads();
            if (threadIdx.x < 3) {
#pragma unroll 8
                for (int q = 0; q < cnt; q++) sum += sc[threadIdx.x][q];
            }
            __syncthreads();
        }
        if (threadIdx.x < 3) {
            const float v = sum * (1.0f / (float)(j1 - j0));     // (an empty cell: 0 * inf = NaN, exactly as the reference)
            mean[threadIdx.x] = v;
            if (blockIdx.y == 0) c.xc[3 * k + threadIdx.x] = v;
        }
        __syncthreads();
        cx = mean[0]; cy = mean[1]; cz = mean[2];
    } else {
        cx = c.xc[3 * k]; cy = c.xc[3 * k + 1]; cz = c.xc[3 * k + 2];
    }
    // gridDim.z > 1 (big cells, fgt_model_splits): workgroup z takes a contiguous range of the cell's rounds of G tiles and leaves a PARTIAL sum
    // (fgt_model_combine_kernel adds the partials in z order)
    if (gridDim.z > 1) {
        const int rounds = (j1 - j0 + FGT_TILE * G - 1) / (FGT_TILE * G);
        const int per = (rounds + (int)gridDim.z - 1) / (int)gridDim.z;
        const int r0 = min(rounds, (int)blockIdx.z * per), r1 = min(rounds, r0 + per);
        const int lo = j0 + r0 * FGT_TILE * G, hi = min(j1, j0 + r1 * FGT_TILE * G);
        j0 = lo; j1 = max(lo, hi);
    }
    float acc[W];
#pragma unroll
    for (int w = 0; w < W; w++) acc[w] = 0.f;
    for (int base = j0; base < j1; base += FGT_TILE * G) {
        const int mine = base + grp * FGT_TILE;                    // this group's tile of the round
        const int cnt = max(0, min(FGT_TILE, j1 - mine));
        if (tid < cnt) {
            const int i = c.memb[mine + tid];
            float d[3] = {(c.x[i] - cx) * inv_sigma, (c.y[i] - cy) * inv_sigma, (c.z[i] - cz) * inv_sigma};
            const float s = expf(-len2(d[0], d[1], d[2]));
            // the reference multiplies the coordinates onto the seed exp(-|d|^2) and gets exactly 0 when the seed is 0; the powers formed
            // first overflow there once |d| > FLT_MAX^(1/(p-1)) (~379 at p = 16), and 0 * inf would be NaN -- such a member's powers are
            // taken at d = 0 (every product is then +-0, which leaves a sum unchanged; a NaN mean still gives a NaN seed)
            if (s == 0.f) d[0] = d[1] = d[2] = 0.f;
#pragma unroll
            for (int a = 0; a < 3; a++) {
                float pw = 1.0f;
                for (int r = 0; r < t.p; r++) { sp[grp][a][r][tid] = pw; pw = d[a] * pw; }
            }
            se[grp][tid] = s;
            if (W == 4) {
                const float4 w = w4[i];
                sw[grp][0][tid] = w.x; sw[grp][1 % W][tid] = w.y; sw[grp][2 % W][tid] = w.z; sw[grp][3 % W][tid] = w.w;
            }
        }
        __syncthreads();
        if (live) {
            const float* __restrict__ pz = sp[grp][2][ec];
            const float* __restrict__ py = sp[grp][1][eb];
            const float* __restrict__ px = sp[grp][0][ea];
#pragma unroll 4
            for (int q = 0; q < cnt; q++) {
                // exp(-|d|^2) z^c y^b x^a, the factors applied in the recursion's order (z, then y, then x); the powers
                // themselves are formed first, which moves the last bit only
                const float pr = ((se[grp][q] * pz[q]) * py[q]) * px[q];
                if (W == 1) acc[0] += pr;                          // weights of ones (cpdutils.cpp:42)
                else {
#pragma unroll
                    for (int w = 0; w < W; w++) acc[w] += sw[grp][w][q] * pr;
                }
            }
        }
        __syncthreads();
    }
    // the groups' sums, added in group order (the tiles' arrays are free now: their memory carries the hand-over)
    float* comb = &sp[0][0][0][0];                                 // [G][W][FGT_TILE]
    static_assert(sizeof(sp) >= sizeof(float) * G * 4 * FGT_TILE, "the hand-over fits the tile arrays");
#pragma unroll
    for (int w = 0; w < W; w++) comb[(grp * W + w) * FGT_TILE + tid] = acc[w];
    __syncthreads();
    if (grp != 0 || !live) return;
    const float ck = t.ck[m];
    const int h = t.hpos[m];
#pragma unroll
    for (int w = 0; w < W; w++) {
        float tot = comb[w * FGT_TILE + tid];
#pragma unroll
        for (int g2 = 1; g2 < G; g2++) tot += comb[(g2 * W + w) * FGT_TILE + tid];
        // fgt.cpp:299-305; [cell][Horner slot][weight]: the four weights of a slot side by side (gridDim.z > 1: B is the partials' array, [z] outermost)
        B[(((size_t)blockIdx.z * c.K + k) * t.pd + h) * W + w] = tot * ck;
    }
}

// B[i] = part[0][i] + part[1][i] + ... in z order (the big cells' partial sums, see above)
__global__ __launch_bounds__(256) void fgt_model_combine_kernel(const float* __restrict__ part, int Z, size_t count, float* __restrict__ B)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    float tot = part[i];
    for (int z = 1; z < Z; z++) tot += part[(size_t)z * count + i];
    B[i] = tot;
}

// Cell means of BIG cells (thousands of members): fgt_centers_kernel's sums -- sequential fp32 in ascending point order, the reference's bits --
// with the gathers of the next 512 members in flight while lanes 0..2 of the first wave add up the current ones (two LDS buffers, one barrier per round).
__global__ __launch_bounds__(512) void fgt_centers_big_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ z,
                                                              const int* __restrict__ memb, const int* __restrict__ off, float* __restrict__ xc)
{
    constexpr int PER = 4, R = 512 * PER;              // 2 048 members per round: their sums (~4 us) outlast the next round's gathers
    __shared__ float s[2][3][R];
    const int k = blockIdx.x, tid = threadIdx.x;
    const int j0 = off[k], j1 = off[k + 1];
    float sum = 0.f;
#pragma unroll
    for (int r = 0; r < PER; r++) {
        const int q = r * 512 + tid;
        if (j0 + q < j1) { const int i = memb[j0 + q]; s[0][0][q] = x[i]; s[0][1][q] = y[i]; s[0][2][q] = z[i]; }
    }
    __syncthreads();
    int buf = 0;
    for (int base = j0; base < j1; base += R, buf ^= 1) {
        const int cnt = min(R, j1 - base), next = base + R;
        float nx[PER], ny[PER], nz[PER];
#pragma unroll
        for (int r = 0; r < PER; r++) {                                    // (in flight during the sums below)
            const int q = next + r * 512 + tid;
            nx[r] = ny[r] = nz[r] = 0.f;
            if (q < j1) { const int i = memb[q]; nx[r] = x[i]; ny[r] = y[i]; nz[r] = z[i]; }
        }
        if (tid < 3) {
#pragma unroll 8
            for (int q = 0; q < cnt; q++) sum += s[buf][tid][q];
        }
#pragma unroll
        for (int r = 0; r < PER; r++) {
            const int q = r * 512 + tid;
            if (next + q < j1) { s[buf ^ 1][0][q] = nx[r]; s[buf ^ 1][1][q] = ny[r]; s[buf ^ 1][2][q] = nz[r]; }
        }
        __syncthreads();
    }
    if (tid < 3) xc[3 * k + tid] = sum * (1.0f / (float)(j1 - j0));     // (an empty cell: 0 * inf = NaN, exactly as the reference)
}

// ---------------------------------------------------------------------------------------------------------------
// ComputeFGTPredict (fgt.cpp:88-150).  Coefficients of cell k are stored in Horner traversal order:
//   for a = p-1..0, for b = p-1-a..0, for c = p-1-a-b..0   ->  sum_a x^a sum_b y^b sum_c z^c B[a,b,c]
// so the innermost loop is r = r*z + B[h++] with B[h] wave-uniform (scalar loads, batched when P is a compile-time constant).
// ---------------------------------------------------------------------------------------------------------------
// pa[w] = sum_a x^a sum_b y^b sum_c z^c Bk[w][h(a,b,c)]; P > 0: compile-time order, fully unrolled; P == 0: any order.
template <int W, int P>
struct Horner {
    static __device__ __forceinline__ void eval(int, float dx, float dy, float dz, const float* __restrict__ Bk, float (&pa)[W])
    {
        int h = 0;
#pragma unroll
        for (int a = P - 1; a >= 0; a--) {
            float pb[W];
#pragma unroll
            for (int w = 0; w < W; w++) pb[w] = 0.f;
#pragma unroll
            for (int b = P - 1 - a; b >= 0; b--) {
                float pc[W];
#pragma unroll
                for (int w = 0; w < W; w++) pc[w] = 0.f;
#pragma unroll
                for (int cdeg = P - 1 - a - b; cdeg >= 0; cdeg--, h++) {
#pragma unroll
                    for (int w = 0; w < W; w++) pc[w] = __builtin_fmaf(pc[w], dz, Bk[h * W + w]);
                }
#pragma unroll
                for (int w = 0; w < W; w++) pb[w] = __builtin_fmaf(pb[w], dy, pc[w]);
            }
#pragma unroll
            for (int w = 0; w < W; w++) pa[w] = __builtin_fmaf(pa[w], dx, pb[w]);
        }
    }
};

template <int W>
struct Horner<W, 0> {
    static __device__ __forceinline__ void eval(int p, float dx, float dy, float dz, const float* __restrict__ Bk, float (&pa)[W])
    {
        int h = 0;
        for (int a = p - 1; a >= 0; a--) {
            float pb[W];
            for (int w = 0; w < W; w++) pb[w] = 0.f;
            for (int b = p - 1 - a; b >= 0; b--) {
                float pc[W];
                for (int w = 0; w < W; w++) pc[w] = 0.f;
                for (int cdeg = p - 1 - a - b; cdeg >= 0; cdeg--, h++)
                    for (int w = 0; w < W; w++) pc[w] = __builtin_fmaf(pc[w], dz, Bk[h * W + w]);
                for (int w = 0; w < W; w++) pb[w] = __builtin_fmaf(pb[w], dy, pc[w]);
            }
            for (int w = 0; w < W; w++) pa[w] = __builtin_fmaf(pa[w], dx, pb[w]);
        }
    }
};

template <int W, int P>
__global__ __launch_bounds__(64) void fgt_predict_kernel(const float* __restrict__ qx, const float* __restrict__ qy,
                                                          const float* __restrict__ qz, int nq, const float* __restrict__ xc,
                                                          const float* __restrict__ B, int K, int pd, int p_runtime, float inv_sigma,
                                                          float e_param, float* __restrict__ v)
{
    // grid = (queries / 64, S): one wave per workgroup, and the cells are split S ways (partial sums, added in a fixed order by
    // the post kernels), so that bunny-sized clouds still put several waves on every SIMD
    const int i = blockIdx.x * 64 + threadIdx.x;
    const int S = gridDim.y, split = blockIdx.y;
    const int k_begin = (int)((long long)K * split / S), k_end = (int)((long long)K * (split + 1) / S);
    const int ic = min(i, nq - 1);
    const float x = qx[ic], y = qy[ic], z = qz[ic];
    float cell[W];
#pragma unroll
    for (int w = 0; w < W; w++) cell[w] = 0.f;
    for (int k = k_begin; k < k_end; k++) {
        const float dx = (x - xc[3 * k]) * inv_sigma, dy = (y - xc[3 * k + 1]) * inv_sigma, dz = (z - xc[3 * k + 2]) * inv_sigma;
        const float sum = len2(dx, dy, dz);
        if (sum > e_param) continue;                               // fgt.cpp:120 (a NaN cell is not skipped there either)
        const float e = expf(-sum);
        float pa[W];
#pragma unroll
        for (int w = 0; w < W; w++) pa[w] = 0.f;
        Horner<W, P>::eval(p_runtime, dx, dy, dz, B + (size_t)k * pd * W, pa);
#pragma unroll
        for (int w = 0; w < W; w++) cell[w] += e * pa[w];
    }
    if (i < nq) {
#pragma unroll
        for (int w = 0; w < W; w++) v[((size_t)split * W + w) * nq + i] = cell[w];
    }
}

// (grid-stride over the points: with xpartials the workgroup count is the M-step's row count -- cpd_xsums_kernel's own mapping, terms and order)
__global__ __launch_bounds__(256) void fgt_post_kt1_kernel(const float* __restrict__ kt1_parts, int S, const float* __restrict__ ax,
                                                           const float* __restrict__ ay, const float* __restrict__ az, int n, float ndi,
                                                           float* __restrict__ pt1, float4* __restrict__ xw4, double* __restrict__ xpartials)
{
    double acc[CPD_XSUMS] = {0};
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        // the S partial sums in split order -- sixteen loads in flight, then the additions in their order (one load per addition waited a round
        // trip each: 59 workgroups of a bunny-sized cloud have nothing else to run meanwhile)
        float kt1 = 0.f;
        for (int sp0 = 0; sp0 < S; sp0 += 16) {
            float part[16];
#pragma unroll
            for (int j = 0; j < 16; j++) part[j] = sp0 + j < S ? kt1_parts[(size_t)(sp0 + j) * n + i] : 0.f;
#pragma unroll
            for (int j = 0; j < 16; j++)
                if (sp0 + j < S) kt1 += part[j];
        }
        const float inv = 1.0f / (kt1 + ndi);                          // cpdutils.cpp:49
        const float x = ax[i], y = ay[i], z = az[i];
        const float p = 1.0f - ndi * inv;                              // CalculatePt1, cpdutils.cpp:79-88
        pt1[i] = p;
        xw4[i] = make_float4(x * inv, y * inv, z * inv, inv);          // CalculateWeightsForPX :90-99; .w doubles as 1/denominator
        if (xpartials != nullptr) {
            acc[0] += (double)logf(1.0f / inv);                         // error -= log(denominator), cpdutils.cpp:69-71
            acc[1] += (double)x * p; acc[2] += (double)y * p; acc[3] += (double)z * p;
            acc[4] += (double)(x * x) * p + (double)(y * y) * p + (double)(z * z) * p;     // coherentpointdrift.cpp:257
        }
    }
    if (xpartials != nullptr) block_sum_store<CPD_XSUMS>(acc, xpartials + (size_t)blockIdx.x * CPD_XSUMS);
}

__global__ __launch_bounds__(256) void fgt_post_px_kernel(const float* __restrict__ v_parts, int S, int m, float* __restrict__ p1,
                                                          float* __restrict__ px, double* __restrict__ kpartials, const float* __restrict__ bx,
                                                          const float* __restrict__ by, const float* __restrict__ bz)
{
    double acc[CPD_KSUMS] = {0};
    for (int k = blockIdx.x * 256 + threadIdx.x; k < m; k += gridDim.x * 256) {
        float a[4] = {0.f, 0.f, 0.f, 0.f};
        for (int sp0 = 0; sp0 < S; sp0 += 8) {                          // (eight splits' loads in flight, added in split order: see fgt_post_kt1_kernel)
            float part[8][4];
#pragma unroll
            for (int j = 0; j < 8; j++)
#pragma unroll
                for (int w = 0; w < 4; w++) part[j][w] = sp0 + j < S ? v_parts[((size_t)(sp0 + j) * 4 + w) * m + k] : 0.f;
#pragma unroll
            for (int j = 0; j < 8; j++)
                if (sp0 + j < S) {
#pragma unroll
                    for (int w = 0; w < 4; w++) a[w] += part[j][w];
                }
        }
        px[3 * (size_t)k] = a[0];
        px[3 * (size_t)k + 1] = a[1];
        px[3 * (size_t)k + 2] = a[2];
        p1[k] = a[3];
        if (kpartials != nullptr) {
            const float b[3] = {bx[k], by[k], bz[k]};
            acc[0] += (double)a[3];
            for (int r = 0; r < 3; r++) {
                acc[1 + r] += (double)b[r] * a[3];
                for (int c = 0; c < 3; c++) acc[4 + 3 * r + c] += (double)b[r] * a[c];
                acc[13] += (double)(b[r] * b[r]) * a[3];                                          // coherentpointdrift.cpp:259
            }
        }
    }
    if (kpartials != nullptr) block_sum_store<CPD_KSUMS>(acc, kpartials + (size_t)blockIdx.x * CPD_KSUMS);
}

// ---------------------------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------------------------
// scratch of the member-list sort: chunk counters H[G][K] (G * K <= 2^22) + the K label totals
constexpr size_t FGT_LIST_MAX_COUNTERS = (size_t)1 << 22;
size_t fgt_sort_temp_bytes(int) { return sizeof(int) * (FGT_LIST_MAX_COUNTERS + 65536 + 16); }

int fgt_replay_points_per_lane(int n) { return n <= 65536 ? 1 : (n <= 262144 ? 4 : 16); }
int fgt_replay_waves(int n) { const int per = 64 * fgt_replay_points_per_lane(n); return (n + per - 1) / per; }
int fgt_replay_limit(int guess, int K) { return guess < 2 ? 0 : std::min(std::min(guess, K), FGT_REPLAY_MAX_CENTRES); }

template <bool ARGMAX>
static void launch_replay(const FgtClusters& c, int lim, const int* limit_ptr, int skip_if_ge, hipStream_t s)
{
    const int P = fgt_replay_points_per_lane(c.n), W = fgt_replay_waves(c.n);
    const size_t lds = sizeof(float4) * (size_t)lim;
#define MI_REPLAY(PP) hipLaunchKernelGGL((fgt_replay_kernel<PP, ARGMAX>), dim3(W), dim3(64), lds, s, c.x, c.y, c.z, c.n, c.picked, lim, limit_ptr, skip_if_ge, \
                                         c.dist, c.indx, c.replay_partial, c.replay_state)
    if (P == 1) MI_REPLAY(1); else if (P == 4) MI_REPLAY(4); else MI_REPLAY(16);
#undef MI_REPLAY
}

static hipError_t launch_replay_and_check(const FgtClusters& c, int lim, hipStream_t s)
{
    launch_replay<true>(c, lim, nullptr, 0, s);
    hipLaunchKernelGGL(fgt_replay_check_kernel, dim3(std::max(1, (lim - 1 + 3) / 4)), dim3(256), 0, s, c.replay_partial, fgt_replay_waves(c.n), c.picked, lim, c.replay_state);
    launch_replay<false>(c, lim, c.replay_state, lim, s);
    return hipGetLastError();
}

hipError_t fgt_replay_prelaunch(const FgtClusters& c, hipStream_t s)
{
    const int lim = c.replay_partial != nullptr && c.replay_state != nullptr ? fgt_replay_limit(c.guess, c.K) : 0;
    return lim > 0 ? launch_replay_and_check(c, lim, s) : hipErrorInvalidValue;
}

// The cooperative sweep, if the cloud fits it and the device takes the launch; false: the caller's other paths.
static bool launch_coop_sweep(const FgtClusters& c, int start, const int* start_ptr, hipStream_t s)
{
    const int enabled = c.coop_sweep;
    if (enabled == 0 || c.sweep_scratch == nullptr || c.n > FGT_COOP_MAX_POINTS) return false;
    // a cooperative launch costs more than a plain one and does not overlap another stream's: it pays for a sweep of many steps (a cloud's first
    // clustering), not for the one or two centres a later E-step adds behind a verified replay (measured: CPD at 49 000 points, hybrid, 8 iterations:
    // 2.92 ms without it, 3.22 ms with it on every sweep)
    if (enabled != 2 && (start_ptr != nullptr || c.K - start < FGT_COOP_MIN_STEPS)) return false;
    static int supported = -1;
    if (supported < 0) {
        int dev = 0, v = 0;
        supported = hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&v, hipDeviceAttributeCooperativeLaunch, dev) == hipSuccess && v != 0 ? 1 : 0;
    }
    if (supported == 0) return false;
    int per = 1;
    while (per < 16 && (long long)FGT_COOP_MAX_GROUPS * 1024 * per < c.n) per *= 2;
    const int G = (c.n + 1024 * per - 1) / (1024 * per);
    unsigned int* counter = reinterpret_cast<unsigned int*>(c.sweep_scratch);
    CoopSlot* slots = reinterpret_cast<CoopSlot*>(reinterpret_cast<unsigned char*>(c.sweep_scratch) + 64);
    if (hipMemsetAsync(counter, 0, sizeof(unsigned int), s) != hipSuccess) return false;
    const float *x = c.x, *y = c.y, *z = c.z;
    int n = c.n, K = c.K;
    float* dist = c.dist;
    int *indx = c.indx, *picked = c.picked;
    void* args[] = {&x, &y, &z, &n, &start, &start_ptr, &K, &dist, &indx, &picked, &counter, &slots};
    const void* fn = per == 1 ? reinterpret_cast<const void*>(fgt_kcenter_coop_kernel<1>) : per == 2 ? reinterpret_cast<const void*>(fgt_kcenter_coop_kernel<2>)
                   : per == 4 ? reinterpret_cast<const void*>(fgt_kcenter_coop_kernel<4>) : per == 8 ? reinterpret_cast<const void*>(fgt_kcenter_coop_kernel<8>)
                   : reinterpret_cast<const void*>(fgt_kcenter_coop_kernel<16>);
    if (hipLaunchCooperativeKernel(fn, dim3(G), dim3(1024), args, 0, s) != hipSuccess) { (void)hipGetLastError(); return false; }
    return true;
}

hipError_t fgt_cluster(const FgtClusters& c, void* sort_temp, size_t sort_temp_bytes, hipStream_t s)
{
    int start = c.k_done > 0 && c.k_done < c.K ? c.k_done : 0;
    const int* start_ptr = nullptr;
    const int lim = start == 0 && c.replay_partial != nullptr && c.replay_state != nullptr ? fgt_replay_limit(c.guess, c.K) : 0;
    if (lim > 0) {
        // the guess replayed and checked (fgt_replay_kernel); what it leaves: dist / indx after state[0] verified steps
        hipError_t e = c.replay_done ? hipSuccess : launch_replay_and_check(c, lim, s);
        if (e != hipSuccess) return e;
        start_ptr = c.replay_state;
        if (c.n > FGT_GRID_SWEEP_MIN_POINTS) {                        // the grid-wide sweep is driven from the host: it needs the number
            e = hipMemcpyAsync(&start, c.replay_state, sizeof(int), hipMemcpyDeviceToHost, s);
            if (e == hipSuccess) e = hipStreamSynchronize(s);
            if (e != hipSuccess) return e;
            start_ptr = nullptr;
        }
    }
    if (start_ptr == nullptr && start >= c.K) { /* every step replayed and verified */ }
    else if (c.n > 16 * 1024 && launch_coop_sweep(c, start, start_ptr, s)) { /* several workgroups, one launch (fgt_kcenter_coop_kernel) */ }
    else if (c.n > FGT_GRID_SWEEP_MIN_POINTS && c.sweep_scratch != nullptr) {
        // large clouds: one grid-wide launch per step (update + per-workgroup arg-max) and a one-workgroup pick in between --
        // two launches per centre instead of one workgroup streaming the whole cloud K times
        ArgMax* cur = reinterpret_cast<ArgMax*>(c.sweep_scratch);
        ArgMax* partials = cur + 1;
        int G = (c.n + 256 * 8 - 1) / (256 * 8);
        if (G > FGT_GRID_SWEEP_BLOCKS) G = FGT_GRID_SWEEP_BLOCKS;
        if (start > 0) hipLaunchKernelGGL(fgt_sweep_step_kernel, dim3(G), dim3(256), 0, s, c.x, c.y, c.z, c.n, cur, 0, 1, c.dist, c.indx, partials, c.picked);
        for (int step = start; step < c.K; step++) {
            if (step > 0) hipLaunchKernelGGL(fgt_sweep_pick_kernel, dim3(1), dim3(256), 0, s, partials, G, cur, c.picked + step);
            hipLaunchKernelGGL(fgt_sweep_step_kernel, dim3(G), dim3(256), 0, s, c.x, c.y, c.z, c.n, cur, step, 0, c.dist, c.indx, partials, c.picked);
        }
    }
    else if (c.n <= 4 * 1024) hipLaunchKernelGGL(fgt_kcenter_kernel<4>, dim3(1), dim3(1024), 0, s, c.x, c.y, c.z, c.n, start, start_ptr, c.K, c.dist, c.indx, c.picked);
    else if (c.n <= 16 * 1024) hipLaunchKernelGGL(fgt_kcenter_kernel<16>, dim3(1), dim3(1024), 0, s, c.x, c.y, c.z, c.n, start, start_ptr, c.K, c.dist, c.indx, c.picked);
    else hipLaunchKernelGGL(fgt_kcenter_kernel<0>, dim3(1), dim3(1024), 0, s, c.x, c.y, c.z, c.n, start, start_ptr, c.K, c.dist, c.indx, c.picked);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (lists_in_model(c)) return hipSuccess;    // (fgt_model(..., centers = true) lists them itself)
    // member lists (stable counting sort on the labels, see fgt_lists_pass_kernel)
    int chunk = 64, G = (c.n + chunk - 1) / chunk;                // one step per wave while the counters fit
    while (G > 4096 || (size_t)G * (size_t)c.K > FGT_LIST_MAX_COUNTERS) { chunk *= 2; G = (c.n + chunk - 1) / chunk; }
    if (sort_temp_bytes < sizeof(int) * ((size_t)G * c.K + c.K + 1)) return hipErrorInvalidValue;
    int* H = reinterpret_cast<int*>(sort_temp);
    int* tot = H + (size_t)G * c.K;
    int label_bits = 1;
    while ((1 << label_bits) < c.K) label_bits++;
    const bool lds = c.K <= FGT_LIST_LDS_LABELS, scan_off = c.K <= FGT_LIST_SCAN_LABELS;
    if (!lds) {
        e = hipMemsetAsync(H, 0, sizeof(int) * (size_t)G * c.K, s);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((fgt_lists_pass_kernel<false, false>), dim3(G), dim3(64), lds ? sizeof(int) * (size_t)c.K : 0, s, c.indx, c.n, c.K, chunk, label_bits, H, nullptr, nullptr, nullptr);
    hipLaunchKernelGGL(fgt_lists_columns_kernel, dim3((c.K + 3) / 4), dim3(256), 0, s, H, G, c.K, tot);
    if (scan_off)
        hipLaunchKernelGGL((fgt_lists_pass_kernel<true, true>), dim3(G), dim3(64), sizeof(int) * (2 * (size_t)c.K + 1), s, c.indx, c.n, c.K, chunk, label_bits, H, tot, c.off, c.memb);
    else {
        hipLaunchKernelGGL(fgt_lists_offsets_kernel, dim3(1), dim3(1024), 0, s, tot, c.K, c.off);
        hipLaunchKernelGGL((fgt_lists_pass_kernel<true, false>), dim3(G), dim3(64), lds ? sizeof(int) * (size_t)c.K : 0, s, c.indx, c.n, c.K, chunk, label_bits, H, tot, c.off, c.memb);
    }
    if (!c.centers_in_model) {
        if (c.n / c.K >= 2048) hipLaunchKernelGGL(fgt_centers_big_kernel, dim3(c.K), dim3(512), 0, s, c.x, c.y, c.z, c.memb, c.off, c.xc);   // (the same sums, for big cells)
        else hipLaunchKernelGGL(fgt_centers_kernel, dim3(c.K), dim3(FGT_TILE), 0, s, c.x, c.y, c.z, c.memb, c.off, c.K, c.xc);
    }
    return hipGetLastError();
}

// Big cells: with n / K in the thousands a workgroup per cell leaves most of the chip idle (10^6 points, 51 cells: 0.9 ms per build).  The rounds of a
// cell's member list are then split over Z workgroups (partial sums, added in z order by a small kernel).  1 for every cloud the bunny-sized tests
// run: their bits do not move.
int fgt_model_splits(int n, int K, int pd)
{
    const int ny = (pd + FGT_TILE - 1) / FGT_TILE;
    const long long per_cell = (long long)n / (K > 0 ? K : 1);
    long long Z = per_cell / (FGT_TILE * FGT_MODEL_GROUPS);                // at least one round of G tiles per workgroup
    const long long fill = 1024 / ((long long)K * ny > 0 ? (long long)K * ny : 1);   // ... and no more than ~1 024 workgroups in all
    if (Z > fill) Z = fill;
    if (Z > FGT_MODEL_MAX_SPLITS) Z = FGT_MODEL_MAX_SPLITS;
    return Z < 1 ? 1 : (int)Z;
}

hipError_t fgt_model(const FgtClusters& c, const float4* w4, float sigma, const FgtTables& t, float* B, hipStream_t s, bool centers, float* part, int Z)
{
    const float inv = 1.0f / sigma;                                // fgt.cpp:260
    if (part != nullptr && Z > 1 && !lists_in_model(c)) {
        const dim3 gridz(c.K, (t.pd + FGT_TILE - 1) / FGT_TILE, Z);
        if (centers) hipLaunchKernelGGL(fgt_centers_big_kernel, dim3(c.K), dim3(512), 0, s, c.x, c.y, c.z, c.memb, c.off, c.xc);
        if (w4) hipLaunchKernelGGL((fgt_model_kernel<4, false, false>), gridz, dim3(FGT_TILE * FGT_MODEL_GROUPS), 0, s, c, w4, inv, t, part);
        else hipLaunchKernelGGL((fgt_model_kernel<1, false, false>), gridz, dim3(FGT_TILE * FGT_MODEL_GROUPS), 0, s, c, w4, inv, t, part);
        const size_t count = (size_t)c.K * t.pd * (w4 ? 4 : 1);
        hipLaunchKernelGGL(fgt_model_combine_kernel, dim3((unsigned int)((count + 255) / 256)), dim3(256), 0, s, part, Z, count, B);
        return hipGetLastError();
    }
    const dim3 grid(c.K, (t.pd + FGT_TILE - 1) / FGT_TILE);
    if (centers && lists_in_model(c)) {
        if (w4) hipLaunchKernelGGL((fgt_model_kernel<4, true, true>), grid, dim3(FGT_TILE * FGT_MODEL_GROUPS), 0, s, c, w4, inv, t, B);
        else hipLaunchKernelGGL((fgt_model_kernel<1, true, true>), grid, dim3(FGT_TILE * FGT_MODEL_GROUPS), 0, s, c, w4, inv, t, B);
    } else if (centers) {
        if (w4) hipLaunchKernelGGL((fgt_model_kernel<4, true, false>), grid, dim3(FGT_TILE * FGT_MODEL_GROUPS), 0, s, c, w4, inv, t, B);
        else hipLaunchKernelGGL((fgt_model_kernel<1, true, false>), grid, dim3(FGT_TILE * FGT_MODEL_GROUPS), 0, s, c, w4, inv, t, B);
    } else {
        if (w4) hipLaunchKernelGGL((fgt_model_kernel<4, false, false>), grid, dim3(FGT_TILE * FGT_MODEL_GROUPS), 0, s, c, w4, inv, t, B);
        else hipLaunchKernelGGL((fgt_model_kernel<1, false, false>), grid, dim3(FGT_TILE * FGT_MODEL_GROUPS), 0, s, c, w4, inv, t, B);
    }
    return hipGetLastError();
}

// ways to split the cells of one transform: enough waves for ~4 per SIMD, at most 16 and at most one cell per split
int fgt_predict_splits(int nq, int K)
{
    const int waves = (nq + 63) / 64;
    int S = (4096 + waves - 1) / waves;
    if (S > 16) S = 16;
    if (S > K) S = K;
    return S < 1 ? 1 : S;
}

hipError_t fgt_predict(const float* qx, const float* qy, const float* qz, int nq, const float* xc, const float* B, int K, int W,
                       float sigma, float e_param, const FgtTables& t, int S, float* v, hipStream_t s)
{
    const float inv = 1.0f / sigma;                                // fgt.cpp:98
    const dim3 grid((nq + 63) / 64, S);
#define MISLAM_PREDICT(WW, PP) \
    hipLaunchKernelGGL((fgt_predict_kernel<WW, PP>), grid, dim3(64), 0, s, qx, qy, qz, nq, xc, B, K, t.pd, t.p, inv, e_param, v)
    if (t.p == 8) { if (W == 4) MISLAM_PREDICT(4, 8); else MISLAM_PREDICT(1, 8); }
    else { if (W == 4) MISLAM_PREDICT(4, 0); else MISLAM_PREDICT(1, 0); }
#undef MISLAM_PREDICT
    return hipGetLastError();
}

hipError_t fgt_post_kt1(const float* kt1_parts, int S, const float* ax, const float* ay, const float* az, int n, float ndi, float* pt1,
                        float4* xw4, hipStream_t s, double* xpartials, int nblocks)
{
    const int blocks = xpartials != nullptr ? nblocks : (n + 255) / 256;
    hipLaunchKernelGGL(fgt_post_kt1_kernel, dim3(blocks), dim3(256), 0, s, kt1_parts, S, ax, ay, az, n, ndi, pt1, xw4, xpartials);
    return hipGetLastError();
}

hipError_t fgt_post_px(const float* v_parts, int S, int m, float* p1, float* px, hipStream_t s, double* kpartials, int nblocks, const float* bx,
                       const float* by, const float* bz)
{
    const int blocks = kpartials != nullptr ? nblocks : (m + 255) / 256;
    hipLaunchKernelGGL(fgt_post_px_kernel, dim3(blocks), dim3(256), 0, s, v_parts, S, m, p1, px, kpartials, bx, by, bz);
    return hipGetLastError();
}

}  // namespace mislam

// Touching one kernel of this translation unit makes the runtime load its code object now (mi_ctx_create) instead of at the
// first launch inside a registration call (deferred loading: 5-16 ms per object, once).
namespace mislam {
__global__ void preload_cpd_fgt_kernel() {}
hipError_t preload_cpd_fgt()
{
    hipFuncAttributes attr;
    return hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(preload_cpd_fgt_kernel));
}
}  // namespace mislam
