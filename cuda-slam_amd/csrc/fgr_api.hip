// mi_fgr_register, mi_fgr_tuples and mi_fgr_system behind the C ABI, up to the step kernel's arguments: argument checks, the matches by
// rank gathered on the host (the index array is the host's: one pass over it checks and lists), the reserves of the call's own buffers
// in the context, both clouds' upload, range pass and input check (knn_check_inputs: the pass of cloud_range.hpp that every search opens
// with) and their one read-back, the tuple trials and their compaction (outlier_compact) with its one read-back, the gather of the used
// list.  The state block, the iterations in batches of sync_every between host reads of the state, and the results are the pose loop's
// (pose_loop.hip), which gets the step's launch; the weights pass and the used list's download follow the loop.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "context.h"
#include "fgr_schedule.hpp"

using namespace mislam;

extern "C" void mi_fgr_params_default(mi_fgr_params* p)
{
    if (!p) return;
    std::memset(p, 0, sizeof *p);
    p->max_distance = 0.f;             // the caller must set it
    p->division_factor = 1.4f;
    p->decrease_every = 4;
    p->max_iterations = 64;
    p->tuple_scale = 0.95f;
    p->max_tuples = 1000;
    p->tuple_trials = 0;
    p->seed = 0;
    p->eps_rotation = 0.f;
    p->eps_translation = 0.f;
    p->sync_every = 0;
}

namespace {

static_assert(2 * sizeof(KnnState) <= 64 * sizeof(float), "two KnnStates must fit the context's pinned scratch");

// what the checks leave for the call: the matches by rank and the numbers the kernels take
struct FgrSetup {
    int C = 0, trials = 0, used_max = 0;
    std::vector<int> match_src, match_tgt;
    double e2 = 0.0, delta2 = 0.0, division_factor = 0.0;
};

// what the prepared call knows: the used list's length, the accepted trials, the scale and the centre
struct FgrPlan {
    int used = 0, accepted = 0;
    double D2 = 0.0;
    float centre[3] = {0.f, 0.f, 0.f};
};

// the checks all three entry points share; nothing has been written or launched when it refuses
int fgr_check(mi_ctx* c, const char* who, const float* src_xyz, int n, const float* tgt_xyz, int m, const int* idx, const mi_fgr_params* p, const float* T,
              FgrSetup* out)
{
    if (!c) { set_error("%s: null context", who); return MI_ERR_INVALID_ARG; }
    if (!src_xyz || !tgt_xyz || !idx || !p) { set_error("%s: null src_xyz, tgt_xyz, idx or params", who); return MI_ERR_INVALID_ARG; }
    if (n < 1 || m < 1) { set_error("%s: empty cloud (n = %d, m = %d)", who, n, m); return MI_ERR_INVALID_ARG; }
    if (!(p->max_distance > 0.f) || !std::isfinite(p->max_distance)) { set_error("%s: max_distance %g is not a positive finite number", who, (double)p->max_distance); return MI_ERR_INVALID_ARG; }
    if (!(p->division_factor > 1.f) || !std::isfinite(p->division_factor)) { set_error("%s: division_factor %g is not a finite number above 1", who, (double)p->division_factor); return MI_ERR_INVALID_ARG; }
    if (p->decrease_every < 1) { set_error("%s: decrease_every = %d below 1", who, p->decrease_every); return MI_ERR_INVALID_ARG; }
    if (!(p->tuple_scale >= 0.f && p->tuple_scale < 1.f)) { set_error("%s: tuple_scale %g outside [0, 1)", who, (double)p->tuple_scale); return MI_ERR_INVALID_ARG; }
    if (p->max_tuples < 1 || p->max_tuples > MI_FGR_MAX_TUPLES) { set_error("%s: max_tuples = %d outside [1, %d]", who, p->max_tuples, MI_FGR_MAX_TUPLES); return MI_ERR_INVALID_ARG; }
    if (p->tuple_trials < 0 || p->tuple_trials > MI_RANSAC_MAX_HYPOTHESES) { set_error("%s: tuple_trials = %d outside [0, %d]", who, p->tuple_trials, MI_RANSAC_MAX_HYPOTHESES); return MI_ERR_INVALID_ARG; }
    const PoseLoopFields loop{p->eps_rotation, p->eps_translation, p->max_iterations, p->sync_every, p->verbose, "terms"};
    MI_TRY(pose_check_fields(who, loop));
    MI_TRY(pose_check_transform(who, T));
    if (c->distributed()) { set_error("%s: single-GPU contexts only", who); return MI_ERR_STATE; }
    out->match_src.clear(); out->match_tgt.clear();
    for (int i = 0; i < n; i++) {
        const int j = idx[i];
        if (j >= m || j < -1) { set_error("%s: idx[%d] = %d is neither -1 nor inside [0, %d)", who, i, j, m); return MI_ERR_INVALID_ARG; }
        if (j < 0) continue;
        out->match_src.push_back(i); out->match_tgt.push_back(j);
    }
    out->C = (int)out->match_src.size();
    if (out->C < 3) { set_error("%s: %d correspondences, fewer than 3", who, out->C); return MI_ERR_INVALID_ARG; }
    out->e2 = (double)p->tuple_scale * (double)p->tuple_scale;
    out->delta2 = (double)p->max_distance * (double)p->max_distance;
    out->division_factor = (double)p->division_factor;
    const long long all = std::min<long long>(100LL * out->C, MI_RANSAC_MAX_HYPOTHESES);
    out->trials = p->tuple_scale > 0.f ? (p->tuple_trials > 0 ? p->tuple_trials : (int)all) : 0;
    out->used_max = p->tuple_scale > 0.f ? 3 * std::min(out->trials, p->max_tuples) : out->C;
    return MI_OK;
}

// one cloud: upload, AoS -> SoA and packed, the range pass into *state (the SoA arrays and the partials are scratch: one stream, in order)
int fgr_upload_cloud(mi_ctx* c, const float* xyz, int count, float4* packed, KnnState* state)
{
    mi_ctx::FgrBuffers& b = c->fgr;
    MI_TRY(host_to_device(c, b.staging.p, xyz, sizeof(float) * 3 * (size_t)count));
    MI_HIP(aos_to_soa(b.staging.p, count, count, b.x.p, b.y.p, b.z.p, packed, c->stream));
    MI_HIP(knn_check_inputs(b.x.p, b.y.p, b.z.p, count, nullptr, nullptr, nullptr, 0, b.range_lo_hi.p, b.range_bad.p, state, c->stream));
    return MI_OK;
}

// Stages 0 - 4 of every call: after it the used list is on the device (plan->used entries; 0: no trial was accepted) and checked against
// the buffers.  want_loop: the rows, slabs and state of the pose loop are reserved beside the call's own.
int fgr_prepare(mi_ctx* c, const char* who, StageClock& clock, CallBuffers& bufs, const float* src_xyz, int n, const float* tgt_xyz, int m,
                const mi_fgr_params* p, const FgrSetup& su, bool want_loop, bool want_weights, FgrPlan* plan)
{
    mi_ctx::FgrBuffers& b = c->fgr;
    const size_t np = (size_t)n, mp = (size_t)m, C = (size_t)su.C, H = (size_t)su.trials, U = (size_t)su.used_max;
    MI_TRY(bufs.need(b.staging, 3 * std::max(np, mp))); MI_TRY(bufs.need(b.x, std::max(np, mp))); MI_TRY(bufs.need(b.y, std::max(np, mp)));
    MI_TRY(bufs.need(b.z, std::max(np, mp))); MI_TRY(bufs.need(b.src4, np)); MI_TRY(bufs.need(b.tgt4, mp));
    MI_TRY(bufs.need(b.range_lo_hi, 2 * 6 * (size_t)KNN_RANGE_BLOCKS)); MI_TRY(bufs.need(b.range_bad, 2 * (size_t)KNN_RANGE_BLOCKS)); MI_TRY(bufs.need(b.kstate, 2));
    MI_TRY(bufs.need(b.match_src, C)); MI_TRY(bufs.need(b.match_tgt, C));
    if (H > 0) {
        MI_TRY(bufs.need(b.triples, 3 * H)); MI_TRY(bufs.need(b.accept, H)); MI_TRY(bufs.need(b.kept_trials, H));
        MI_TRY(bufs.need(b.tile_counts, (size_t)outlier_scan_tiles(su.trials))); MI_TRY(bufs.need(b.ostate, 1));
    }
    MI_TRY(bufs.need(b.used_src, U)); MI_TRY(bufs.need(b.used_tgt, U)); MI_TRY(bufs.need(b.used_p, U)); MI_TRY(bufs.need(b.used_q, U));
    MI_TRY(bufs.need(b.mu, 1));
    if (want_weights) MI_TRY(bufs.need(b.weights, U));
    if (want_loop) MI_TRY(pose_loop_reserve(b.loop, su.used_max, false));
    MI_TRY(clock.mark(0));

    MI_TRY(fgr_upload_cloud(c, src_xyz, n, b.src4.p, b.kstate.p));
    MI_TRY(fgr_upload_cloud(c, tgt_xyz, m, b.tgt4.p, b.kstate.p + 1));
    MI_TRY(host_to_device(c, b.match_src.p, su.match_src.data(), sizeof(int) * C));
    MI_TRY(host_to_device(c, b.match_tgt.p, su.match_tgt.data(), sizeof(int) * C));
    MI_TRY(clock.mark(1));
    KnnState* st = reinterpret_cast<KnnState*>(c->h_scratch);      // (pinned, 256 bytes)
    MI_HIP(hipMemcpyAsync(st, b.kstate.p, 2 * sizeof(KnnState), hipMemcpyDeviceToHost, c->stream));
    MI_HIP(hipStreamSynchronize(c->stream));
    MI_TRY(clock.mark(2));
    // everything that can refuse the input is known here, before any output array has been touched
    if (st[0].bad_cloud != KNN_NO_POINT) { set_error("%s: src_xyz point %d has a non-finite coordinate or one above 1e18 in magnitude", who, st[0].bad_cloud); return MI_ERR_INVALID_ARG; }
    if (st[1].bad_cloud != KNN_NO_POINT) { set_error("%s: tgt_xyz point %d has a non-finite coordinate or one above 1e18 in magnitude", who, st[1].bad_cloud); return MI_ERR_INVALID_ARG; }
    plan->D2 = std::max(fgr_diagonal2(st[0].lo, st[0].hi), fgr_diagonal2(st[1].lo, st[1].hi));
    for (int i = 0; i < 3; i++) plan->centre[i] = 0.5f * (st[1].lo[i] + st[1].hi[i]);

    // host-side shape checks before the hand-written kernels run: every array they index is as long as the launches assume
    if (!bufs.fits() || (want_loop && !pose_loop_fits(b.loop, su.used_max, false))) { set_error("internal: %s buffers shorter than the launch", who); return MI_ERR_STATE; }
    plan->accepted = 0;
    plan->used = su.C;
    if (su.trials > 0) {
        FgrTrialArgs ta{};
        ta.src4 = b.src4.p; ta.tgt4 = b.tgt4.p; ta.match_src = b.match_src.p; ta.match_tgt = b.match_tgt.p; ta.C = su.C;
        ta.seed = p->seed; ta.e2 = su.e2; ta.trials = su.trials; ta.triples = b.triples.p; ta.accept = b.accept.p;
        MI_HIP(fgr_trials(ta, c->stream));               // (not booked to a profiling slot: "nn" and "solve" hold the iterations' two launches alone)
        OutlierCompactArgs ca{};
        ca.keep = b.accept.p; ca.n = su.trials; ca.tile_counts = b.tile_counts.p; ca.out_index = b.kept_trials.p; ca.state = b.ostate.p;
        MI_HIP(outlier_compact(ca, c->stream));
        MI_TRY(compact_read_state(c, b.ostate.p, 1));
        MI_HIP(hipStreamSynchronize(c->stream));
        long long kept = 0;
        if (!compact_kept(c, 0, su.trials, &kept)) { set_error("internal: %s accepted %lld of %d trials", who, kept, su.trials); return MI_ERR_STATE; }
        plan->accepted = (int)kept;
        plan->used = 3 * std::min(plan->accepted, p->max_tuples);
    }
    MI_TRY(clock.mark(3));
    if (plan->used > su.used_max) { set_error("internal: %s lists %d used matches, more than the %d reserved", who, plan->used, su.used_max); return MI_ERR_STATE; }
    if (plan->used > 0) {
        FgrGatherArgs ga{};
        ga.src4 = b.src4.p; ga.tgt4 = b.tgt4.p; ga.match_src = b.match_src.p; ga.match_tgt = b.match_tgt.p;
        ga.kept_trials = su.trials > 0 ? b.kept_trials.p : nullptr; ga.triples = su.trials > 0 ? b.triples.p : nullptr;
        ga.used = plan->used; ga.used_src = b.used_src.p; ga.used_tgt = b.used_tgt.p; ga.used_p = b.used_p.p; ga.used_q = b.used_q.p;
        MI_HIP(fgr_gather(ga, c->stream));
    }
    return clock.mark(4);
}

FgrStepArgs fgr_step_args(mi_ctx* c, const mi_fgr_params* p, const FgrSetup& su, const FgrPlan& plan, int k)
{
    mi_ctx::FgrBuffers& b = c->fgr;
    FgrStepArgs a{};
    a.state = b.loop.state.p; a.p = b.used_p.p; a.q = b.used_q.p; a.used = plan.used;
    a.D2 = plan.D2; a.delta2 = su.delta2; a.division_factor = su.division_factor; a.decrease_every = p->decrease_every; a.k = k;
    a.rows = b.loop.rows.p; a.mu_out = b.mu.p; a.weights = nullptr;
    return a;
}

}  // namespace

extern "C" int mi_fgr_register(mi_ctx* c, const float* src_xyz, int n, const float* tgt_xyz, int m, const int* idx, const mi_fgr_params* p,
                               const float init_T[16], float out_T[16], int* iterations, float* error, int* stop_reason, int* used, float* final_mu,
                               float* weights, int* used_src)
{
    const char* who = "mi_fgr_register";
    FgrSetup su;
    if (c && (!out_T || !used)) { set_error("%s: null out_T or used", who); return MI_ERR_INVALID_ARG; }
    MI_TRY(fgr_check(c, who, src_xyz, n, tgt_xyz, m, idx, p, init_T, &su));
    const PoseLoopFields loop{p->eps_rotation, p->eps_translation, p->max_iterations, p->sync_every, p->verbose, "terms"};
    MI_ENTER(c);
    mi_ctx::FgrBuffers& b = c->fgr;
    StageClock clock(c, b.ms);         // mi_fgr_register_times
    CallBuffers bufs;
    FgrPlan plan;
    MI_TRY(fgr_prepare(c, who, clock, bufs, src_xyz, n, tgt_xyz, m, p, su, true, weights != nullptr, &plan));

    PlaneState h;
    if (plan.used == 0) {              // no trial was accepted: the start pose, and nothing ran
        pose_state_at(init_T, plan.centre, &h);
        h.done = 1; h.stop_reason = MI_STOP_NO_PAIRS;
    } else {
        MI_TRY(pose_loop_upload_state(c, b.loop, clock, init_T, plan.centre, &h));
        const FgrStepArgs a = fgr_step_args(c, p, su, plan, -1);
        MI_TRY(pose_loop_run(c, b.loop, clock, who, plan.used, loop, &h, [&] { return fgr_step(a, c->stream); }));
    }
    const bool behind_update = h.stop_reason == MI_STOP_CONVERGED || h.stop_reason == MI_STOP_MAX_ITERATIONS;
    const int last_k = fgr_last_k(h.iterations, behind_update);
    if (plan.used > 0 && (weights || used_src)) {
        if (weights) {
            FgrStepArgs a = fgr_step_args(c, p, su, plan, last_k);
            a.weights = b.weights.p;
            MI_HIP(fgr_weights(a, c->stream));
            MI_HIP(hipMemcpyAsync(weights, b.weights.p, sizeof(float) * (size_t)plan.used, hipMemcpyDeviceToHost, c->stream));
        }
        if (used_src) MI_HIP(hipMemcpyAsync(used_src, b.used_src.p, sizeof(int) * (size_t)plan.used, hipMemcpyDeviceToHost, c->stream));
        MI_HIP(hipStreamSynchronize(c->stream));
    }
    *used = plan.used;
    if (final_mu) *final_mu = (float)fgr_mu(plan.D2, su.delta2, su.division_factor, p->decrease_every, last_k);
    return pose_loop_results(clock, h, out_T, iterations, error, stop_reason);
}

extern "C" int mi_fgr_tuples(mi_ctx* c, const float* src_xyz, int n, const float* tgt_xyz, int m, const int* idx, const mi_fgr_params* p, int* used,
                             int* used_src, int* used_tgt, int* accepted_trials)
{
    const char* who = "mi_fgr_tuples";
    FgrSetup su;
    if (c && !used) { set_error("%s: null used", who); return MI_ERR_INVALID_ARG; }
    MI_TRY(fgr_check(c, who, src_xyz, n, tgt_xyz, m, idx, p, nullptr, &su));
    MI_ENTER(c);
    mi_ctx::FgrBuffers& b = c->fgr;
    double ms[8];
    StageClock clock(c, ms);
    CallBuffers bufs;
    FgrPlan plan;
    MI_TRY(fgr_prepare(c, who, clock, bufs, src_xyz, n, tgt_xyz, m, p, su, false, false, &plan));
    if (plan.used > 0) {
        if (used_src) MI_HIP(hipMemcpyAsync(used_src, b.used_src.p, sizeof(int) * (size_t)plan.used, hipMemcpyDeviceToHost, c->stream));
        if (used_tgt) MI_HIP(hipMemcpyAsync(used_tgt, b.used_tgt.p, sizeof(int) * (size_t)plan.used, hipMemcpyDeviceToHost, c->stream));
    }
    MI_HIP(hipStreamSynchronize(c->stream));
    *used = plan.used;
    if (accepted_trials) *accepted_trials = plan.accepted;
    return MI_OK;
}

extern "C" int mi_fgr_system(mi_ctx* c, const float* src_xyz, int n, const float* tgt_xyz, int m, const int* idx, const mi_fgr_params* p, const float T[16],
                             int applied_updates, double out_sums[32], float out_centre[3], double* mu)
{
    const char* who = "mi_fgr_system";
    FgrSetup su;
    if (c && !out_sums) { set_error("%s: null out_sums", who); return MI_ERR_INVALID_ARG; }
    if (c && applied_updates < 0) { set_error("%s: applied_updates = %d is negative", who, applied_updates); return MI_ERR_INVALID_ARG; }
    MI_TRY(fgr_check(c, who, src_xyz, n, tgt_xyz, m, idx, p, T, &su));
    MI_ENTER(c);
    mi_ctx::FgrBuffers& b = c->fgr;
    StageClock clock(c, b.ms);         // mi_fgr_register_times
    CallBuffers bufs;
    FgrPlan plan;
    MI_TRY(fgr_prepare(c, who, clock, bufs, src_xyz, n, tgt_xyz, m, p, su, true, false, &plan));

    PlaneState h;
    double mu_host = fgr_mu(plan.D2, su.delta2, su.division_factor, p->decrease_every, applied_updates);
    if (plan.used == 0) {
        pose_state_at(T, plan.centre, &h);
    } else {
        MI_TRY(pose_loop_upload_state(c, b.loop, clock, T, plan.centre, &h));
        const FgrStepArgs a = fgr_step_args(c, p, su, plan, applied_updates);
        MI_TRY(pose_loop_system_run(c, b.loop, clock, plan.used, &h, nullptr, [&] { return fgr_step(a, c->stream); }));
        MI_HIP(hipMemcpyAsync(&mu_host, b.mu.p, sizeof(double), hipMemcpyDeviceToHost, c->stream));      // the device's own
    }
    MI_TRY(pose_loop_system_finish(c, clock, h, out_sums, out_centre));
    if (mu) *mu = mu_host;
    return MI_OK;
}

extern "C" int mi_fgr_register_times(mi_ctx* c, double out_ms[MI_FGR_STAGES]) { return stage_times("mi_fgr_register_times", c ? c->fgr.ms : nullptr, out_ms); }
