// mi_evaluate_registration behind the C ABI, modelled on plane_api.hip: argument checks, the reserves of the call's own buffers in the context,
// the search front end with the fixed cloud as the cloud and the moving cloud as the queries (search_front.hip: uploads, input check and
// its one read-back, the cell grid under mi_knn_search's points-per-cell rule for k = 1, the curve order of the moving cloud), the state
// block at the pose, one launch of K55's step (eval_kernels.hip) and K16's rows reduce through the pose loop's *_system half
// (pose_loop.hip), and the host arithmetic behind the sums (eval_block.hpp).  With the pairs given, pair_idx is uploaded and checked on the
// device beside the clouds (its refusal is read back behind the front end's own) and no grid is built; the curve order is still taken, so
// that a moving point sits in the same row of the sums in both modes.
#include <hip/hip_runtime.h>

#include <cmath>

#include "context.h"
#include "eval_block.hpp"

using namespace mislam;

extern "C" int mi_evaluate_registration(mi_ctx* c, const float* before_xyz, int n, const float* after_xyz, int m, const float T[16], const int* pair_idx,
                                        int dist_mode, float max_distance_squared, double* out_fitness, double* out_inlier_rmse, double out_sums[32],
                                        double out_information[36], int* out_idx, float* out_d2)
{
    const char* who = "mi_evaluate_registration";
    if (!c) { set_error("%s: null context", who); return MI_ERR_INVALID_ARG; }
    if (!before_xyz || !after_xyz) { set_error("%s: null before_xyz or after_xyz", who); return MI_ERR_INVALID_ARG; }
    if (!out_fitness || !out_inlier_rmse) { set_error("%s: null out_fitness or out_inlier_rmse", who); return MI_ERR_INVALID_ARG; }
    if (n < 1 || m < 1) { set_error("%s: empty moving or fixed cloud (n = %d, m = %d)", who, n, m); return MI_ERR_INVALID_ARG; }
    if (dist_mode != MI_DIST_CPU_ROUNDING && dist_mode != MI_DIST_FMA) { set_error("%s: bad dist_mode %d", who, dist_mode); return MI_ERR_INVALID_ARG; }
    if (!(max_distance_squared >= 0.f)) { set_error("%s: max_distance_squared %g is NaN or negative", who, (double)max_distance_squared); return MI_ERR_INVALID_ARG; }
    MI_TRY(pose_check_transform(who, T));
    if (c->distributed()) { set_error("%s: single-GPU contexts only", who); return MI_ERR_STATE; }
    MI_ENTER(c);
    mi_ctx::EvalBuffers& b = c->eval;
    StageClock clock(c, b.ms);         // mi_evaluate_registration_times

    const bool given = pair_idx != nullptr, want_idx = out_idx != nullptr;
    const size_t np = (size_t)n, mp = (size_t)m;
    CallBuffers bufs;
    MI_TRY(search_front_reserve(b.front, np, mp, false));
    MI_TRY(bufs.result(b.out_d2, np, out_d2));
    if (given) { MI_TRY(bufs.need(b.pair_idx, np)); MI_TRY(bufs.need(b.pair_bad, 1)); }
    MI_TRY(pose_loop_reserve(b.loop, n, want_idx));
    MI_TRY(clock.mark(0));

    // the pairs go first: uploaded and checked while the clouds are on their way (one stream: in order)
    int bad = KNN_NO_POINT;
    if (given) {
        MI_TRY(host_to_device(c, b.pair_bad.p, &bad, sizeof bad));
        MI_TRY(host_to_device(c, b.pair_idx.p, pair_idx, sizeof(int) * np));
        MI_HIP(eval_check_pairs(b.pair_idx.p, n, m, b.pair_bad.p, c->stream));
    }
    SearchFront f;
    MI_TRY(search_front_upload_and_check(c, b.front, clock, who, after_xyz, m, before_xyz, n, &f, "after_xyz", "before_xyz"));
    if (given) {
        MI_HIP(hipMemcpyAsync(&bad, b.pair_bad.p, sizeof bad, hipMemcpyDeviceToHost, c->stream));
        MI_HIP(hipStreamSynchronize(c->stream));
        MI_TRY(clock.mark(2));
        if (bad != KNN_NO_POINT) {
            set_error("%s: pair_idx entry %d is %d, neither -1 nor a fixed index in [0, %d)", who, bad, pair_idx[bad], m);
            return MI_ERR_INVALID_ARG;
        }
        MI_TRY(search_front_order(c, b.front, clock, &f));
        // (no grid: what search_front_fits would ask of the front end's buffers, without the cells)
        MI_TRY(bufs.watch(b.front.qx, np)); MI_TRY(bufs.watch(b.front.qy, np)); MI_TRY(bufs.watch(b.front.qz, np)); MI_TRY(bufs.watch(b.front.order, np));
        MI_TRY(bufs.watch(b.front.cx, mp)); MI_TRY(bufs.watch(b.front.cy, mp)); MI_TRY(bufs.watch(b.front.cz, mp));
    } else {
        const float ppc = c->tune.knn_points_per_cell > 0.f ? c->tune.knn_points_per_cell : knn_default_points_per_cell(1);   // mi_knn_search's grid for k = 1
        MI_TRY(search_front_index_and_order(c, b.front, clock, who, ppc, &f));
    }

    float centre[3];                   // (the state block's; K55 takes its moments about the origin and does not read it)
    for (int i = 0; i < 3; i++) centre[i] = 0.5f * (f.bbox[i] + f.bbox[3 + i]);
    PlaneState h;
    MI_TRY(pose_loop_upload_state(c, b.loop, clock, T, centre, &h));

    EvalStepArgs a{};
    a.state = b.loop.state.p;
    a.q = search_front_queries(b.front, f);
    a.c = search_front_cloud(b.front);
    a.pair_idx = given ? b.pair_idx.p : nullptr;
    a.m = m;
    a.max_d2 = max_distance_squared;
    a.rows = b.loop.rows.p;
    a.idx = want_idx ? b.loop.out_idx.p : nullptr;
    a.d2 = out_d2 ? b.out_d2.p : nullptr;
    // host-side shape checks before the hand-written kernels run: every array they index is as long as the launches assume
    if ((!given && !search_front_fits(b.front, f)) || !bufs.fits() || !pose_loop_fits(b.loop, n, want_idx)) {
        set_error("internal: %s buffers shorter than the launch", who);
        return MI_ERR_STATE;
    }

    const int fma = dist_mode == MI_DIST_FMA;
    MI_TRY(pose_loop_system_run(c, b.loop, clock, n, &h, out_idx, [&] { return eval_step(f.g, a, fma, c->stream); }));
    MI_TRY(bufs.download(c->stream));
    double sums[PLANE_ROW];
    MI_TRY(pose_loop_system_finish(c, clock, h, sums, nullptr));

    *out_fitness = eval_fitness(sums, n);
    *out_inlier_rmse = eval_inlier_rmse(sums);
    if (out_sums)
        for (int i = 0; i < PLANE_ROW; i++) out_sums[i] = sums[i];
    if (out_information) eval_information(sums, out_information);
    return MI_OK;
}

extern "C" int mi_evaluate_registration_times(mi_ctx* c, double out_ms[MI_EVAL_STAGES])
{
    return stage_times("mi_evaluate_registration_times", c ? c->eval.ms : nullptr, out_ms);
}
