// mi_estimate_covariances, mi_icp_gicp_register and mi_gicp_system behind the C ABI.  The covariance call is mi_estimate_normals' driver with
// another kernel and result (normals_kernels.hip: the same search and moments).  The registration, up to the step kernel's arguments: argument
// checks, the reserves of the call's own buffers in the context, the covariances' upload, repack and input check (gicp_kernels.hip), the search
// front end with the fixed cloud as the cloud and the moving cloud as the queries (search_front.hip), the moving cloud's covariances along its
// curve order.  The state block, the iterations -- the step of gicp_kernels.hip, then plane_kernels.hip's own reduce and solve -- in batches of
// sync_every between host reads of the state, and the results are the pose loop's (pose_loop.hip), which gets the step's launch.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "context.h"

using namespace mislam;

extern "C" int mi_estimate_covariances(mi_ctx* c, const float* cloud_xyz, int n, int k, int dist_mode, float max_distance_squared, int mode, float epsilon,
                                       float* cov6, int* count)
{
    const char* who = "mi_estimate_covariances";
    if (!c) { set_error("%s: null context", who); return MI_ERR_INVALID_ARG; }
    if (!cloud_xyz || !cov6) { set_error("%s: null cloud_xyz or cov6", who); return MI_ERR_INVALID_ARG; }
    if (n < 1) { set_error("%s: empty cloud (n = %d)", who, n); return MI_ERR_INVALID_ARG; }
    if (k < 2 || k > MI_KNN_MAX_K) { set_error("%s: k = %d outside [2, %d]", who, k, MI_KNN_MAX_K); return MI_ERR_INVALID_ARG; }
    if (dist_mode != MI_DIST_CPU_ROUNDING && dist_mode != MI_DIST_FMA) { set_error("%s: bad dist_mode %d", who, dist_mode); return MI_ERR_INVALID_ARG; }
    if (!(max_distance_squared >= 0.f)) { set_error("%s: max_distance_squared %g is NaN or negative", who, (double)max_distance_squared); return MI_ERR_INVALID_ARG; }
    if (mode != MI_COV_RAW && mode != MI_COV_PLANE) { set_error("%s: bad mode %d", who, mode); return MI_ERR_INVALID_ARG; }
    if (mode == MI_COV_PLANE && !(epsilon >= 0.f && epsilon <= 1.f)) { set_error("%s: epsilon %g is not in [0, 1]", who, (double)epsilon); return MI_ERR_INVALID_ARG; }
    if (c->distributed()) { set_error("%s: single-GPU contexts only", who); return MI_ERR_STATE; }
    MI_ENTER(c);
    mi_ctx::CovarianceBuffers& b = c->cov;
    StageClock clock(c, b.ms);

    const size_t np = (size_t)n;
    CallBuffers bufs;
    MI_TRY(search_front_reserve(b.front, np, np, true));
    MI_TRY(bufs.result(b.out_cov, 6 * np, cov6)); MI_TRY(bufs.result(b.out_count, np, count));
    MI_TRY(clock.mark(0));

    SearchFront f;
    MI_TRY(search_front_upload_and_check(c, b.front, clock, who, cloud_xyz, n, nullptr, n, &f));
    const float ppc = c->tune.knn_points_per_cell > 0.f ? c->tune.knn_points_per_cell : knn_default_points_per_cell(k);   // mi_knn_search's grid, cell size included
    MI_TRY(search_front_index_and_order(c, b.front, clock, who, ppc, &f));

    KnnCovariancesArgs a{};
    const SearchQueries q = search_front_queries(b.front, f);
    const SearchCloud cl = search_front_cloud(b.front);
    a.qx = q.x; a.qy = q.y; a.qz = q.z; a.order = q.order;      // (the kernel keeps the fields of its own: kernels.h)
    a.cx = cl.x; a.cy = cl.y; a.cz = cl.z;
    a.n = q.n; a.k = k; a.max_d2 = max_distance_squared;
    for (int i = 0; i < 3; i++) a.hi[i] = q.hi[i];
    a.plane = mode == MI_COV_PLANE ? 1 : 0;
    a.epsilon = a.plane ? (double)epsilon : 0.0;
    a.cov6 = b.out_cov.p; a.count = count ? b.out_count.p : nullptr;
    // host-side shape checks before the hand-written kernel runs: every array it indexes is as long as the launch assumes
    if (!search_front_fits(b.front, f) || !bufs.fits()) {
        set_error("internal: %s buffers shorter than the launch", who);
        return MI_ERR_STATE;
    }
    MI_TRY(search_front_timed_launch(c, b.front, clock, [&] { return knn_covariances(f.g, a, dist_mode == MI_DIST_FMA, c->stream); }));

    MI_TRY(bufs.download(c->stream));
    MI_HIP(hipStreamSynchronize(c->stream));
    MI_TRY(clock.mark(6));
    clock.finish();
    return MI_OK;
}

namespace {

// what both entry points refuse alike, before the context is touched
int check_arguments(const char* who, mi_ctx* c, const float* before_xyz, const float* before_cov6, int n, const float* after_xyz, const float* after_cov6, int m,
                    int dist_mode, float max_d2, const float* T)
{
    if (!c) { set_error("%s: null context", who); return MI_ERR_INVALID_ARG; }
    if (!before_xyz || !before_cov6 || !after_xyz || !after_cov6) { set_error("%s: null before_xyz, before_cov6, after_xyz or after_cov6", who); return MI_ERR_INVALID_ARG; }
    if (n < 1 || m < 1) { set_error("%s: empty moving or fixed cloud (n = %d, m = %d)", who, n, m); return MI_ERR_INVALID_ARG; }
    if (dist_mode != MI_DIST_CPU_ROUNDING && dist_mode != MI_DIST_FMA) { set_error("%s: bad dist_mode %d", who, dist_mode); return MI_ERR_INVALID_ARG; }
    if (!(max_d2 >= 0.f)) { set_error("%s: max_distance_squared %g is NaN or negative", who, (double)max_d2); return MI_ERR_INVALID_ARG; }
    return pose_check_transform(who, T);
}

// Stages 0 - 4 of either call and the state block at pose T: after it the step kernel's arguments are complete and checked against the buffers.
int gicp_prepare(mi_ctx* c, const char* who, StageClock& clock, const float* before_xyz, const float* before_cov6, int n, const float* after_xyz,
                 const float* after_cov6, int m, float max_d2, const float* T, bool want_idx, SearchFront* f, GicpStepArgs* a, PlaneState* h)
{
    mi_ctx::GicpBuffers& b = c->gicp;
    const size_t np = (size_t)n, mp = (size_t)m;
    CallBuffers bufs;
    MI_TRY(search_front_reserve(b.front, np, mp, false));
    MI_TRY(bufs.need(b.cov_staging, 6 * std::max(np, mp)));
    MI_TRY(bufs.need(b.cov_a, 2 * mp)); MI_TRY(bufs.need(b.cov_b_in, 2 * np)); MI_TRY(bufs.need(b.cov_b, 2 * np)); MI_TRY(bufs.need(b.cov_bad, 2));
    MI_TRY(pose_loop_reserve(b.loop, n, want_idx));
    MI_TRY(clock.mark(0));

    // the covariances go first, each cloud's through the staging buffer (one stream: in order), repacked and checked in one pass
    int bad[2] = {KNN_NO_POINT, KNN_NO_POINT};
    MI_TRY(host_to_device(c, b.cov_bad.p, bad, sizeof bad));
    MI_TRY(host_to_device(c, b.cov_staging.p, before_cov6, sizeof(float) * 6 * np));
    MI_HIP(gicp_pack_covariances(b.cov_staging.p, n, b.cov_b_in.p, b.cov_bad.p, c->stream));
    MI_TRY(host_to_device(c, b.cov_staging.p, after_cov6, sizeof(float) * 6 * mp));
    MI_HIP(gicp_pack_covariances(b.cov_staging.p, m, b.cov_a.p, b.cov_bad.p + 1, c->stream));
    MI_TRY(search_front_upload_and_check(c, b.front, clock, who, after_xyz, m, before_xyz, n, f, "after_xyz", "before_xyz"));
    MI_HIP(hipMemcpyAsync(bad, b.cov_bad.p, sizeof bad, hipMemcpyDeviceToHost, c->stream));
    MI_HIP(hipStreamSynchronize(c->stream));
    MI_TRY(clock.mark(2));
    if (bad[0] != KNN_NO_POINT) {
        set_error("%s: before_cov6 covariance %d has a non-finite entry or one above 1e18 in magnitude", who, bad[0]);
        return MI_ERR_INVALID_ARG;
    }
    if (bad[1] != KNN_NO_POINT) {
        set_error("%s: after_cov6 covariance %d has a non-finite entry or one above 1e18 in magnitude", who, bad[1]);
        return MI_ERR_INVALID_ARG;
    }
    const float ppc = c->tune.knn_points_per_cell > 0.f ? c->tune.knn_points_per_cell : knn_default_points_per_cell(1);   // mi_knn_search's grid for k = 1
    MI_TRY(search_front_index_and_order(c, b.front, clock, who, ppc, f));
    *a = GicpStepArgs{};
    a->q = search_front_queries(b.front, *f);
    a->c = search_front_cloud(b.front);
    MI_HIP(gicp_permute_covariances(b.cov_b_in.p, a->q.order, n, b.cov_b.p, c->stream));
    MI_TRY(clock.mark(4));

    float centre[3];
    for (int i = 0; i < 3; i++) centre[i] = 0.5f * (f->bbox[i] + f->bbox[3 + i]);
    MI_TRY(pose_loop_upload_state(c, b.loop, clock, T, centre, h));

    a->state = b.loop.state.p;
    a->cov_a = b.cov_a.p; a->cov_b = b.cov_b.p;
    a->max_d2 = max_d2;
    a->rows = b.loop.rows.p;
    a->idx = want_idx ? b.loop.out_idx.p : nullptr;
    // host-side shape checks before the hand-written kernels run: every array they index is as long as the launches assume
    if (!search_front_fits(b.front, *f) || !bufs.fits() || !pose_loop_fits(b.loop, n, want_idx)) {
        set_error("internal: %s buffers shorter than the launch", who);
        return MI_ERR_STATE;
    }
    return MI_OK;
}

}  // namespace

extern "C" int mi_icp_gicp_register(mi_ctx* c, const float* before_xyz, const float* before_cov6, int n, const float* after_xyz, const float* after_cov6, int m,
                                    const mi_plane_params* p, const float init_T[16], float out_T[16], int* iterations, float* error, int* stop_reason)
{
    const char* who = "mi_icp_gicp_register";
    if (c && (!p || !out_T)) { set_error("%s: null params or out_T", who); return MI_ERR_INVALID_ARG; }
    MI_TRY(check_arguments(who, c, before_xyz, before_cov6, n, after_xyz, after_cov6, m, p ? p->dist_mode : 0, p ? p->max_distance_squared : 0.f, init_T));
    const PoseLoopFields loop{p->eps_rotation, p->eps_translation, p->max_iterations, p->sync_every, p->verbose, "pairs"};
    MI_TRY(pose_check_fields(who, loop));
    if (c->distributed()) { set_error("%s: single-GPU contexts only", who); return MI_ERR_STATE; }
    MI_ENTER(c);
    mi_ctx::GicpBuffers& b = c->gicp;
    StageClock clock(c, b.ms);         // mi_icp_gicp_times

    SearchFront f;
    GicpStepArgs a;
    PlaneState h;
    MI_TRY(gicp_prepare(c, who, clock, before_xyz, before_cov6, n, after_xyz, after_cov6, m, p->max_distance_squared, init_T, false, &f, &a, &h));

    const int fma = p->dist_mode == MI_DIST_FMA;
    MI_TRY(pose_loop_run(c, b.loop, clock, who, n, loop, &h, [&] { return gicp_step(f.g, a, fma, c->stream); }));
    return pose_loop_results(clock, h, out_T, iterations, error, stop_reason);
}

extern "C" int mi_gicp_system(mi_ctx* c, const float* before_xyz, const float* before_cov6, int n, const float* after_xyz, const float* after_cov6, int m,
                              const float T[16], int dist_mode, float max_distance_squared, double out_sums[32], float out_centre[3], int* out_idx)
{
    const char* who = "mi_gicp_system";
    if (c && !out_sums) { set_error("%s: null out_sums", who); return MI_ERR_INVALID_ARG; }
    MI_TRY(check_arguments(who, c, before_xyz, before_cov6, n, after_xyz, after_cov6, m, dist_mode, max_distance_squared, T));
    if (c->distributed()) { set_error("%s: single-GPU contexts only", who); return MI_ERR_STATE; }
    MI_ENTER(c);
    mi_ctx::GicpBuffers& b = c->gicp;
    StageClock clock(c, b.ms);         // mi_icp_gicp_times

    SearchFront f;
    GicpStepArgs a;
    PlaneState h;
    MI_TRY(gicp_prepare(c, who, clock, before_xyz, before_cov6, n, after_xyz, after_cov6, m, max_distance_squared, T, out_idx != nullptr, &f, &a, &h));

    const int fma = dist_mode == MI_DIST_FMA;
    MI_TRY(pose_loop_system_run(c, b.loop, clock, n, &h, out_idx, [&] { return gicp_step(f.g, a, fma, c->stream); }));
    return pose_loop_system_finish(c, clock, h, out_sums, out_centre);
}

extern "C" int mi_icp_gicp_times(mi_ctx* c, double out_ms[MI_GICP_STAGES]) { return stage_times("mi_icp_gicp_times", c ? c->gicp.ms : nullptr, out_ms); }
