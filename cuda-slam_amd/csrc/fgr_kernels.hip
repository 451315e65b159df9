// K44 - K47 -- Fast Global Registration over correspondences (mi_fgr_register, mi_fgr_tuples, mi_fgr_system; driver: fgr_api.hip; the
// contract: mi_slam.h).  Zhou, Park, Koltun (ECCV 2016): a Geman-McClure objective over ALL matches, its line process eliminated, minimised
// by Gauss-Newton steps while mu anneals from the clouds' scale down to the caller's distance.
//   K44 fgr_trials:  one lane per trial.  K23's three counter-based draws and its edge rule (ransac_draw.hpp, shared, not copied) with
//                    e2 = tuple_scale^2; writes the three RANKS and the accept flag.  The flags go through K15's outlier_compact.
//   K45 fgr_gather:  one lane per used match: the kept trials' draws in draw order (or rank u itself without a filter) -> the match's two
//                    indices and its two points, by used rank.  The step then streams its operands; nothing is gathered per iteration.
//   K46 fgr_step:    one lane per used match, one wave per workgroup, no LDS, as K16 / K17 / K31.  The lane moves its source point with the
//                    state block's fp64 pose (not rounded to fp32: this differs from pose_move), forms r, u, l and hands pose_row_write
//                    (pose_step.hpp) one entry at a time; it keeps u, r, l and mu alive and no accumulator.  mu comes from
//                    state->iterations by fgr_mu (fgr_schedule.hpp) ONCE per lane, in front of the entries: no host round trip, and
//                    nothing of the schedule on the entries' path.  The rows are K16's: plane_reduce_solve stands behind them unchanged.
//   K47 fgr_weights: the step's arithmetic up to l under the state's pose at a given k, one float per used match; no rows, no update.
// No floating-point atomics, no scratch: the same input and seed give the same bits on every call.
#include <hip/hip_runtime.h>

#include "fgr_schedule.hpp"
#include "kernels.h"
#include "pose_step.hpp"
#include "ransac_draw.hpp"

namespace mislam {

namespace {

__global__ __launch_bounds__(FGR_BLOCK) void fgr_trials_kernel(const FgrTrialArgs a)
{
    const int h = blockIdx.x * FGR_BLOCK + threadIdx.x;
    if (h >= a.trials) return;
    unsigned int rank[3];
    for (int r = 0; r < 3; r++) rank[r] = ransac_draw_rank(a.seed, (unsigned long long)h, r, a.C);      // < C
    float s[3][3], t[3][3];
    for (int r = 0; r < 3; r++) {
        const float4 p = a.src4[a.match_src[rank[r]]], q = a.tgt4[a.match_tgt[rank[r]]];
        s[r][0] = p.x; s[r][1] = p.y; s[r][2] = p.z;
        t[r][0] = q.x; t[r][1] = q.y; t[r][2] = q.z;
        a.triples[3 * (size_t)h + r] = (int)rank[r];
    }
    const bool distinct = rank[0] != rank[1] && rank[0] != rank[2] && rank[1] != rank[2];
    a.accept[h] = distinct && ransac_edges_similar(s, t, a.e2) ? 1 : 0;
}

__global__ __launch_bounds__(FGR_BLOCK) void fgr_gather_kernel(const FgrGatherArgs a)
{
    const int u = blockIdx.x * FGR_BLOCK + threadIdx.x;
    if (u >= a.used) return;
    const int rank = a.kept_trials ? a.triples[3 * (size_t)a.kept_trials[u / 3] + (u % 3)] : u;
    const int i = a.match_src[rank], j = a.match_tgt[rank];
    a.used_src[u] = i; a.used_tgt[u] = j;
    a.used_p[u] = a.src4[i]; a.used_q[u] = a.tgt4[j];
}

// What a used match contributes at the pose of *st under mu: u = x - c0, r = x - q, d2 = |r|^2, w = mu / (mu + d2), l = w w.  False, and
// nothing written, where x = R p + t is not finite.
__device__ __forceinline__ bool fgr_term(const PlaneState* __restrict__ st, const float4 pf, const float4 qf, double mu, double (&u)[3], double (&r)[3],
                                         double& d2, double& w, double& l)
{
    const double px = (double)pf.x, py = (double)pf.y, pz = (double)pf.z;
    const double x0 = ((st->R[0] * px + st->R[1] * py) + st->R[2] * pz) + st->t[0];
    const double x1 = ((st->R[3] * px + st->R[4] * py) + st->R[5] * pz) + st->t[1];
    const double x2 = ((st->R[6] * px + st->R[7] * py) + st->R[8] * pz) + st->t[2];
    const double inf = (double)__builtin_inff();
    if (!(__builtin_fabs(x0) < inf && __builtin_fabs(x1) < inf && __builtin_fabs(x2) < inf)) return false;      // (false for NaN)
    r[0] = x0 - (double)qf.x; r[1] = x1 - (double)qf.y; r[2] = x2 - (double)qf.z;
    u[0] = x0 - st->c0[0]; u[1] = x1 - st->c0[1]; u[2] = x2 - st->c0[2];
    d2 = (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2];
    w = mu / (mu + d2);
    l = w * w;
    return true;
}

__global__ __launch_bounds__(KNN_BLOCK) void fgr_step_kernel(const FgrStepArgs a)
{
    const PlaneState* __restrict__ st = a.state;
    if (st->done != 0) return;
    const int lane = (int)threadIdx.x;
    const int s = blockIdx.x * KNN_BLOCK + lane;
    const double mu = fgr_mu(a.D2, a.delta2, a.division_factor, a.decrease_every, a.k >= 0 ? a.k : st->iterations);
    if (blockIdx.x == 0 && lane == 0) a.mu_out[0] = mu;

    double u[3] = {0.0, 0.0, 0.0}, r[3] = {0.0, 0.0, 0.0}, d2 = 0.0, l = 0.0, e = 0.0, count = 0.0;
    if (s < a.used) {
        double uu[3], rr[3], dd, w, ll;
        if (fgr_term(st, a.p[s], a.q[s], mu, uu, rr, dd, w, ll)) {
            for (int i = 0; i < 3; i++) { u[i] = uu[i]; r[i] = rr[i]; }
            d2 = dd; l = ll; count = 1.0;
            const double wm = w - 1.0;
            e = l * d2 + mu * (wm * wm);
        }
    }
    // the three rows of the Jacobian of x about c0: rotation (u crossed in), then translation
    const double Jx[6] = {0.0, u[2], -u[1], 1.0, 0.0, 0.0}, Jy[6] = {-u[2], 0.0, u[0], 0.0, 1.0, 0.0}, Jz[6] = {u[1], -u[0], 0.0, 0.0, 0.0, 1.0};
    pose_row_write(
        lane, a.rows + (size_t)blockIdx.x * PLANE_ROW, [&](int i, int j) { return l * ((Jx[i] * Jx[j] + Jy[i] * Jy[j]) + Jz[i] * Jz[j]); },
        [&](int i) { return l * ((Jx[i] * r[0] + Jy[i] * r[1]) + Jz[i] * r[2]); }, e, d2, count);
}

__global__ __launch_bounds__(FGR_BLOCK) void fgr_weights_kernel(const FgrStepArgs a)
{
    const int s = blockIdx.x * FGR_BLOCK + threadIdx.x;
    if (s >= a.used) return;
    const double mu = fgr_mu(a.D2, a.delta2, a.division_factor, a.decrease_every, a.k);
    double u[3], r[3], d2, w, l = 0.0;
    if (!fgr_term(a.state, a.p[s], a.q[s], mu, u, r, d2, w, l)) l = 0.0;
    a.weights[s] = (float)l;
}

}  // namespace

hipError_t fgr_trials(const FgrTrialArgs& a, hipStream_t s)
{
    if (a.C < 3 || a.trials < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fgr_trials_kernel, dim3((a.trials + FGR_BLOCK - 1) / FGR_BLOCK), dim3(FGR_BLOCK), 0, s, a);
    return hipGetLastError();
}

hipError_t fgr_gather(const FgrGatherArgs& a, hipStream_t s)
{
    if (a.used < 1 || (a.kept_trials == nullptr) != (a.triples == nullptr) || (a.kept_trials && a.used % 3 != 0)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fgr_gather_kernel, dim3((a.used + FGR_BLOCK - 1) / FGR_BLOCK), dim3(FGR_BLOCK), 0, s, a);
    return hipGetLastError();
}

hipError_t fgr_step(const FgrStepArgs& a, hipStream_t s)
{
    if (a.used < 1 || a.decrease_every < 1 || !a.rows || !a.mu_out) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fgr_step_kernel, dim3(plane_row_count(a.used)), dim3(KNN_BLOCK), 0, s, a);
    return hipGetLastError();
}

hipError_t fgr_weights(const FgrStepArgs& a, hipStream_t s)
{
    if (a.used < 1 || a.decrease_every < 1 || a.k < 0 || !a.weights) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fgr_weights_kernel, dim3((a.used + FGR_BLOCK - 1) / FGR_BLOCK), dim3(FGR_BLOCK), 0, s, a);
    return hipGetLastError();
}

// loads this translation unit's code object at mi_ctx_preload (kernels.h)
__global__ void preload_fgr_kernels_kernel() {}
hipError_t preload_fgr_kernels()
{
    hipFuncAttributes attr;
    return hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(preload_fgr_kernels_kernel));
}

}  // namespace mislam
