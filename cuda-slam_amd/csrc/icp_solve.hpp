// The one-lane solve of an ICP iteration and what surrounds it, as device functions: the fixed butterfly over the reduced rows, the Kabsch
// solve + composition (K3) and the stop rules (K6).  Shared by the per-launch kernels of icp_kernels.hip and the whole-loop kernel of
// icp_batch.hip, so that both evaluate an iteration with the same instructions in the same order.
#pragma once
#include <hip/hip_runtime.h>

#include "icp_rows.hpp"
#include "kernels.h"
#include "svd3.hpp"

namespace mislam {

// sums[0..18) <- sum of the `count` (<= 64) reduced rows: lane g takes row g, then the fixed butterfly of icp_rows.hpp over the
// wave.  One load round instead of a serial walk down each column.  Call with all 64 threads; sums is LDS, valid after the barrier.
__device__ __forceinline__ void reduce_rows_wave(const double* __restrict__ part, int count, double* __restrict__ sums)
{
    const int lane = threadIdx.x & 63;
    double mom[16], e0 = 0.0, e1 = 0.0;
#pragma unroll
    for (int k = 0; k < 16; k++) mom[k] = 0.0;
    if (lane < count) {
        const double* __restrict__ row = part + (size_t)lane * ICP_ROW;
#pragma unroll
        for (int k = 0; k < 16; k++) mom[k] = row[k];
        e0 = row[16]; e1 = row[17];
    }
    const double x = wave_sum16(mom, lane);
    const double e = wave_sum2(e0, e1, lane);
    if ((lane & 3) == 0) sums[((lane >> 5) & 1) * 8 + ((lane >> 4) & 1) * 4 + ((lane >> 3) & 1) * 2 + ((lane >> 2) & 1)] = x;
    if ((lane & 31) == 0) sums[ICP_MOMENTS + (lane >> 5)] = e;
    __syncthreads();
}

// seq_b / seq_a (MI_SUM_CPU_SEQUENTIAL, else null): cpu-slam's sequential fp32 running sums of the kept pairs; its centroids
// are those sums divided by (float)count (common.cpp:283), and t inherits their rounding.  The cross-covariance keeps the
// fp64 form: replacing the exact centroids by the rounded ones changes H by n*da*db^T, ~1e-9 relative.
__device__ void solve_from_moments(const double* mom, const float* seq_b, const float* seq_a, float Ri[9], float ti[3], bool svd_ieee, const float* seq_H = nullptr)
{
    const double n = mom[0];
    const double inv_n = 1.0 / n;            // (n is a count: one fp64 division instead of six on the one-lane chain)
    const double cbx = mom[1] * inv_n, cby = mom[2] * inv_n, cbz = mom[3] * inv_n;
    const double cax = mom[4] * inv_n, cay = mom[5] * inv_n, caz = mom[6] * inv_n;
    const double ca[3] = {cax, cay, caz}, cb[3] = {cbx, cby, cbz};
    // H = sum (a - ca)(b - cb)^T = sum a b^T - n ca cb^T   (alignedAfter * alignedBefore^T, common.cpp:530)
    Mat3 H;
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) H.a[r][c] = (float)(mom[7 + 3 * r + c] - n * ca[r] * cb[c]);
    // MI_SUM_CPU_SEQUENTIAL (round 6): cpu-slam's OWN matrix -- the points centred in fp32 with its sequential-sum centroids (icp_seq_cross_kernel).  For a
    // well-conditioned H the two differ by ~1e-7 and R by as little; for a RANK-DEFICIENT one -- the first iteration of a registration whose clouds start
    // 20-30 units apart: 20 000 moving points matched to TWO fixed points, singular values 23 064 / 0 / 0 -- the true H leaves R undetermined and what cpu-slam
    // returns is decided by the rounding of its centring (singular values 23 064 / 1.3e-3 / 0 there); the exact matrix above then lands in another basin
    // (the reference's convergence set, rot 0.6 / trans 30: cpu-slam 47 iterations, the exact matrix 100 iterations and 23 away).  A parity mode retraces it.
    if (seq_H != nullptr)
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++) H.a[r][c] = seq_H[3 * r + c];
    const Kabsch3 k = kabsch_rotation<true>(H, svd_ieee);     // (svd3.hpp SvdMath: hardware reciprocals and roots for the rotation parameters)
    // column-major like glm::mat3 (ConvertRotationMatrix, common.cpp:335-346)
    for (int c = 0; c < 3; c++)
        for (int r = 0; r < 3; r++) Ri[3 * c + r] = k.R.a[r][c];
    float fcb[3] = {(float)cbx, (float)cby, (float)cbz};
    float fca[3] = {(float)cax, (float)cay, (float)caz};
    if (seq_b != nullptr) {
        const float fn = (float)n;
        for (int d = 0; d < 3; d++) { fcb[d] = seq_b[d] / fn; fca[d] = seq_a[d] / fn; }
    }
    // t = centroidAfter - R * centroidBefore (common.cpp:549), glm mat3*vec3 operation order
    for (int i = 0; i < 3; i++) ti[i] = fca[i] - ((Ri[i] * fcb[0] + Ri[3 + i] * fcb[1]) + Ri[6 + i] * fcb[2]);
}

// glm mat3 * mat3, column-major operands (include/glm/detail/type_mat3x3.inl operator*)
__device__ void mat3_mul_cm(const float a[9], const float b[9], float out[9])
{
    float r[9];
    for (int c = 0; c < 3; c++)
        for (int rr = 0; rr < 3; rr++) r[3 * c + rr] = (a[rr] * b[3 * c] + a[3 + rr] * b[3 * c + 1]) + a[6 + rr] * b[3 * c + 2];
    for (int i = 0; i < 9; i++) out[i] = r[i];
}

// Kabsch solve of the moments + composition with the running transform (one lane)
__device__ void apply_solve(IcpState* __restrict__ state, const double* mom, int compose_mode, int seq_sums, int svd_ieee)
{
    state->pairs = (int)mom[0];
    if (mom[0] <= 0.0) {   // "if (correspondingPoints.size() == 0) break;"  basicicp.cpp:36
        state->done = 1;
        state->stop_reason = MI_STOP_NO_PAIRS_;
        return;
    }
    float Ri[9], ti[3];
    float seq_b[3], seq_a[3];
    for (int d = 0; d < 3; d++) { seq_b[d] = state->seq_sum_b[d]; seq_a[d] = state->seq_sum_a[d]; }
    float seq_H[9];
    for (int i = 0; i < 9; i++) seq_H[i] = state->seq_H[i];
    solve_from_moments(mom, seq_sums ? seq_b : nullptr, seq_sums ? seq_a : nullptr, Ri, ti, svd_ieee != 0, seq_sums ? seq_H : nullptr);
    for (int i = 0; i < 9; i++) state->Ri[i] = Ri[i];
    for (int i = 0; i < 3; i++) state->ti[i] = ti[i];
    float R[9], t[3];
    for (int i = 0; i < 9; i++) R[i] = state->R[i];
    for (int i = 0; i < 3; i++) t[i] = state->t[i];
    if (compose_mode == 0) {
        // rotationMatrix = Ri * rotationMatrix; translationVector = ti + translationVector  (basicicp.cpp:43-44)
        mat3_mul_cm(Ri, R, R);
        for (int i = 0; i < 3; i++) t[i] = ti[i] + t[i];
    } else {
        // transformationMatrix = Ti * transformationMatrix  (icpcuda.cu:35)
        float nt[3];
        for (int i = 0; i < 3; i++) nt[i] = ((Ri[i] * t[0] + Ri[3 + i] * t[1]) + Ri[6 + i] * t[2]) + ti[i];
        mat3_mul_cm(Ri, R, R);
        for (int i = 0; i < 3; i++) t[i] = nt[i];
    }
    for (int i = 0; i < 9; i++) state->R[i] = R[i];
    for (int i = 0; i < 3; i++) state->t[i] = t[i];
}

// error of the iteration just applied + the stop rules (one lane)
__device__ void finalize_iteration(IcpState* __restrict__ state, double e0, double e1, const IcpRules& rules)
{
    const double e[2] = {e0, e1};
    // cpu-slam: mean over the surviving pairs (common.cpp:267); cuda-slam: sum / after.size() (cudacommon.cu:147)
    const double denom = rules.filter_pairs ? e[1] : (double)rules.m_total;
    float error = (float)(e[0] / denom);
    if (rules.seq_sums) error = state->seq_sum_err / (float)denom;   // cpu-slam's own fp32 running sum / pair count (common.cpp:267)
    state->error = error;
    state->passes += 1;
    if (error < rules.eps) {                                       // basicicp.cpp:52 / icpcuda.cu:40
        state->done = 1;
        state->stop_reason = MI_STOP_CONVERGED_;
        return;
    }
    if (rules.abort_on_increase && error > state->prev_error) {    // icpcuda.cu:43-49
        for (int i = 0; i < 9; i++) state->R[i] = state->prevR[i];
        for (int i = 0; i < 3; i++) state->t[i] = state->prevT[i];
        state->error = state->prev_error;
        state->done = 1;
        state->stop_reason = MI_STOP_ERROR_INCREASED_;
        return;
    }
    for (int i = 0; i < 9; i++) state->prevR[i] = state->R[i];
    for (int i = 0; i < 3; i++) state->prevT[i] = state->t[i];
    state->prev_error = error;
    state->iterations += 1;                                        // basicicp.cpp:57
    if (rules.max_iterations != -1 && state->iterations >= rules.max_iterations) {
        state->done = 1;
        state->stop_reason = MI_STOP_MAX_ITERATIONS_;
    }
}

// K3 + K6, deferred, as one wave runs it: the sums of the `count` reduced rows (part == null: they are already in state->mom / state->err), the
// PREVIOUS iteration's stop rule if its error sums were pending, then -- unless it fired -- the solve and the composition.  The one body behind
// icp_solve_deferred_kernel, icp_reduce_solve_kernel and icp_rows_reduce_solve_kernel (icp_kernels.hip): the same instructions in the same order
// whichever launch carries them.  Call with the 64 threads of the workgroup's first wave and state->done == 0; sums is LDS (ICP_ROW doubles).
__device__ __forceinline__ void solve_deferred_wave(IcpState* __restrict__ state, const double* part, int count, double* sums, int compose_mode,
                                                    const IcpRules& rules, int mark_pending)
{
    if (part != nullptr) reduce_rows_wave(part, count, sums);
    else {
        if (threadIdx.x < ICP_ROW) sums[threadIdx.x] = threadIdx.x < ICP_MOMENTS ? state->mom[threadIdx.x] : state->err[threadIdx.x - ICP_MOMENTS];
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    if (state->err_pending) {            // the previous iteration's error sums have arrived with these moments
        state->err_pending = 0;
        state->err[0] = sums[ICP_MOMENTS];
        state->err[1] = sums[ICP_MOMENTS + 1];
        finalize_iteration(state, sums[ICP_MOMENTS], sums[ICP_MOMENTS + 1], rules);
        if (state->done != 0) return;    // its stop rule fired: nothing of this iteration is applied
    }
    double mom[ICP_MOMENTS];
    for (int i = 0; i < ICP_MOMENTS; i++) { mom[i] = sums[i]; state->mom[i] = sums[i]; }
    apply_solve(state, mom, compose_mode, rules.seq_sums, rules.svd_ieee);
    if (mark_pending && state->done == 0) state->err_pending = 1;
}

}  // namespace mislam
