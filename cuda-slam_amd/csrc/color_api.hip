// mi_estimate_color_gradients, mi_icp_color_register and mi_color_system behind the C ABI.  The gradient call is mi_fpfh_features' driver
// with the intensities beside the normals and another kernel and result (color_kernels.hip: K13's search in self mode, the sums and the
// solve).  The registration, up to the step kernel's arguments, is plane_api.hip's with more beside the fixed cloud's normals: argument
// checks, the reserves of the call's own buffers in the context, the uploads, repack and input check of the intensities and gradients
// (color_kernels.hip), the normals' upload and input check, the search front end with the fixed cloud as the cloud and the moving cloud as
// the queries (search_front.hip), the moving cloud's intensities along its curve order.  The state block, the iterations -- the step of
// color_kernels.hip, then plane_kernels.hip's own reduce and solve -- in batches of sync_every between host reads of the state, and the
// results are the pose loop's (pose_loop.hip), which gets the step's launch.
#include <hip/hip_runtime.h>

#include <cmath>

#include "context.h"

using namespace mislam;

extern "C" int mi_estimate_color_gradients(mi_ctx* c, const float* cloud_xyz, const float* normals_xyz, const float* intensity, int n, int k, int dist_mode,
                                           float max_distance_squared, float* gradients_xyz, int* count)
{
    const char* who = "mi_estimate_color_gradients";
    if (!c) { set_error("%s: null context", who); return MI_ERR_INVALID_ARG; }
    if (!cloud_xyz || !normals_xyz || !intensity || !gradients_xyz) { set_error("%s: null cloud_xyz, normals_xyz, intensity or gradients_xyz", who); return MI_ERR_INVALID_ARG; }
    if (n < 1) { set_error("%s: empty cloud (n = %d)", who, n); return MI_ERR_INVALID_ARG; }
    if (k < 2 || k > MI_KNN_MAX_K) { set_error("%s: k = %d outside [2, %d]", who, k, MI_KNN_MAX_K); return MI_ERR_INVALID_ARG; }
    if (dist_mode != MI_DIST_CPU_ROUNDING && dist_mode != MI_DIST_FMA) { set_error("%s: bad dist_mode %d", who, dist_mode); return MI_ERR_INVALID_ARG; }
    if (!(max_distance_squared >= 0.f)) { set_error("%s: max_distance_squared %g is NaN or negative", who, (double)max_distance_squared); return MI_ERR_INVALID_ARG; }
    if (c->distributed()) { set_error("%s: single-GPU contexts only", who); return MI_ERR_STATE; }
    MI_ENTER(c);
    mi_ctx::ColorGradientBuffers& b = c->colorgrad;
    StageClock clock(c, b.ms);

    const size_t np = (size_t)n;
    CallBuffers bufs;
    MI_TRY(search_front_reserve(b.front, np, np, true));
    MI_TRY(bufs.need(b.nx, np)); MI_TRY(bufs.need(b.ny, np)); MI_TRY(bufs.need(b.nz, np)); MI_TRY(bufs.need(b.nstate, 1));
    MI_TRY(bufs.need(b.intensity, np)); MI_TRY(bufs.need(b.bad, 1));
    MI_TRY(bufs.result(b.out_gradients, 3 * np, gradients_xyz)); MI_TRY(bufs.result(b.out_count, np, count));
    MI_TRY(clock.mark(0));

    int bad = KNN_NO_POINT;
    MI_TRY(host_to_device(c, b.bad.p, &bad, sizeof bad));
    MI_TRY(host_to_device(c, b.intensity.p, intensity, sizeof(float) * np));
    MI_HIP(color_check_values(b.intensity.p, n, b.bad.p, c->stream));
    MI_TRY(search_front_enqueue_normals(c, b.front, normals_xyz, n, b.nx.p, b.ny.p, b.nz.p, nullptr, b.nstate.p));
    SearchFront f;
    MI_TRY(search_front_upload_and_check(c, b.front, clock, who, cloud_xyz, n, nullptr, n, &f));
    MI_TRY(search_front_refuse_normals(c, clock, who, "normals_xyz", b.nstate.p));
    MI_HIP(hipMemcpyAsync(&bad, b.bad.p, sizeof bad, hipMemcpyDeviceToHost, c->stream));
    MI_HIP(hipStreamSynchronize(c->stream));
    MI_TRY(clock.mark(2));
    if (bad != KNN_NO_POINT) {
        set_error("%s: intensity value %d is non-finite or above 1e18 in magnitude", who, bad);
        return MI_ERR_INVALID_ARG;
    }
    const float ppc = c->tune.knn_points_per_cell > 0.f ? c->tune.knn_points_per_cell : knn_default_points_per_cell(k);   // mi_knn_search's grid, cell size included
    MI_TRY(search_front_index_and_order(c, b.front, clock, who, ppc, &f));

    ColorGradientArgs a{};
    a.q = search_front_queries(b.front, f);
    a.c = search_front_cloud(b.front);
    a.nx = b.nx.p; a.ny = b.ny.p; a.nz = b.nz.p;
    a.intensity = b.intensity.p;
    a.k = k; a.max_d2 = max_distance_squared;
    a.gradients = b.out_gradients.p; a.count = count ? b.out_count.p : nullptr;
    // host-side shape checks before the hand-written kernel runs: every array it indexes is as long as the launch assumes
    if (!search_front_fits(b.front, f) || !bufs.fits()) {
        set_error("internal: %s buffers shorter than the launch", who);
        return MI_ERR_STATE;
    }
    MI_TRY(search_front_timed_launch(c, b.front, clock, [&] { return color_gradients(f.g, a, dist_mode == MI_DIST_FMA, c->stream); }));

    MI_TRY(bufs.download(c->stream));
    MI_HIP(hipStreamSynchronize(c->stream));
    MI_TRY(clock.mark(6));
    clock.finish();
    return MI_OK;
}

namespace {

// what the fixed cloud brings beside its points
struct ColorFixed {
    const float *xyz, *normals, *intensity, *gradients;
};

// what both entry points refuse alike, before the context is touched
int check_arguments(const char* who, mi_ctx* c, const float* before_xyz, const float* before_intensity, int n, const ColorFixed& after, int m, int dist_mode,
                    float max_d2, float lambda, const float* T)
{
    if (!c) { set_error("%s: null context", who); return MI_ERR_INVALID_ARG; }
    if (!before_xyz || !before_intensity || !after.xyz || !after.normals || !after.intensity || !after.gradients) {
        set_error("%s: null before_xyz, before_intensity, after_xyz, after_normals_xyz, after_intensity or after_gradients_xyz", who);
        return MI_ERR_INVALID_ARG;
    }
    if (n < 1 || m < 1) { set_error("%s: empty moving or fixed cloud (n = %d, m = %d)", who, n, m); return MI_ERR_INVALID_ARG; }
    if (dist_mode != MI_DIST_CPU_ROUNDING && dist_mode != MI_DIST_FMA) { set_error("%s: bad dist_mode %d", who, dist_mode); return MI_ERR_INVALID_ARG; }
    if (!(max_d2 >= 0.f)) { set_error("%s: max_distance_squared %g is NaN or negative", who, (double)max_d2); return MI_ERR_INVALID_ARG; }
    if (!(lambda >= 0.f && lambda <= 1.f)) { set_error("%s: lambda_geometric %g is NaN or outside [0, 1]", who, (double)lambda); return MI_ERR_INVALID_ARG; }
    return pose_check_transform(who, T);
}

// Stages 0 - 4 of either call and the state block at pose T: after it the step kernel's arguments are complete and checked against the buffers.
int color_prepare(mi_ctx* c, const char* who, StageClock& clock, const float* before_xyz, const float* before_intensity, int n, const ColorFixed& after, int m,
                  float max_d2, float lambda, const float* T, bool want_idx, SearchFront* f, ColorStepArgs* a, PlaneState* h)
{
    mi_ctx::ColorBuffers& b = c->color;
    const size_t np = (size_t)n, mp = (size_t)m;
    CallBuffers bufs;
    MI_TRY(search_front_reserve(b.front, np, mp, false));
    MI_TRY(bufs.need(b.nx, mp)); MI_TRY(bufs.need(b.ny, mp)); MI_TRY(bufs.need(b.nz, mp)); MI_TRY(bufs.need(b.normals, mp)); MI_TRY(bufs.need(b.nstate, 1));
    MI_TRY(bufs.need(b.ia_in, mp)); MI_TRY(bufs.need(b.grad_in, 3 * mp)); MI_TRY(bufs.need(b.grad_i, mp));
    MI_TRY(bufs.need(b.ib_in, np)); MI_TRY(bufs.need(b.ib, np)); MI_TRY(bufs.need(b.bad, 3));
    MI_TRY(pose_loop_reserve(b.loop, n, want_idx));
    MI_TRY(clock.mark(0));

    // the intensities and gradients go first, each into a buffer of its own (one stream: in order), repacked and checked in one pass
    int bad[3] = {KNN_NO_POINT, KNN_NO_POINT, KNN_NO_POINT};
    MI_TRY(host_to_device(c, b.bad.p, bad, sizeof bad));
    MI_TRY(host_to_device(c, b.ib_in.p, before_intensity, sizeof(float) * np));
    MI_HIP(color_check_values(b.ib_in.p, n, b.bad.p, c->stream));
    MI_TRY(host_to_device(c, b.ia_in.p, after.intensity, sizeof(float) * mp));
    MI_TRY(host_to_device(c, b.grad_in.p, after.gradients, sizeof(float) * 3 * mp));
    MI_HIP(color_pack_fixed(b.grad_in.p, b.ia_in.p, m, b.grad_i.p, b.bad.p + 1, b.bad.p + 2, c->stream));
    MI_TRY(search_front_enqueue_normals(c, b.front, after.normals, m, b.nx.p, b.ny.p, b.nz.p, b.normals.p, b.nstate.p));
    MI_TRY(search_front_upload_and_check(c, b.front, clock, who, after.xyz, m, before_xyz, n, f, "after_xyz", "before_xyz"));
    MI_TRY(search_front_refuse_normals(c, clock, who, "after_normals_xyz", b.nstate.p));
    MI_HIP(hipMemcpyAsync(bad, b.bad.p, sizeof bad, hipMemcpyDeviceToHost, c->stream));
    MI_HIP(hipStreamSynchronize(c->stream));
    MI_TRY(clock.mark(2));
    if (bad[0] != KNN_NO_POINT) {
        set_error("%s: before_intensity value %d is non-finite or above 1e18 in magnitude", who, bad[0]);
        return MI_ERR_INVALID_ARG;
    }
    if (bad[1] != KNN_NO_POINT) {
        set_error("%s: after_intensity value %d is non-finite or above 1e18 in magnitude", who, bad[1]);
        return MI_ERR_INVALID_ARG;
    }
    if (bad[2] != KNN_NO_POINT) {
        set_error("%s: after_gradients_xyz gradient %d has a non-finite component or one above 1e18 in magnitude", who, bad[2]);
        return MI_ERR_INVALID_ARG;
    }
    const float ppc = c->tune.knn_points_per_cell > 0.f ? c->tune.knn_points_per_cell : knn_default_points_per_cell(1);   // mi_knn_search's grid for k = 1
    MI_TRY(search_front_index_and_order(c, b.front, clock, who, ppc, f));
    *a = ColorStepArgs{};
    a->q = search_front_queries(b.front, *f);
    a->c = search_front_cloud(b.front);
    MI_HIP(color_permute_intensity(b.ib_in.p, a->q.order, n, b.ib.p, c->stream));
    MI_TRY(clock.mark(4));

    float centre[3];
    for (int i = 0; i < 3; i++) centre[i] = 0.5f * (f->bbox[i] + f->bbox[3 + i]);
    MI_TRY(pose_loop_upload_state(c, b.loop, clock, T, centre, h));

    a->state = b.loop.state.p;
    a->normals = b.normals.p;
    a->grad_i = b.grad_i.p;
    a->ib = b.ib.p;
    a->lambda = (double)lambda;
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

extern "C" int mi_icp_color_register(mi_ctx* c, const float* before_xyz, const float* before_intensity, int n, const float* after_xyz,
                                     const float* after_normals_xyz, const float* after_intensity, const float* after_gradients_xyz, int m,
                                     const mi_plane_params* p, float lambda_geometric, const float init_T[16], float out_T[16], int* iterations, float* error,
                                     int* stop_reason)
{
    const char* who = "mi_icp_color_register";
    if (c && (!p || !out_T)) { set_error("%s: null params or out_T", who); return MI_ERR_INVALID_ARG; }
    const ColorFixed after{after_xyz, after_normals_xyz, after_intensity, after_gradients_xyz};
    MI_TRY(check_arguments(who, c, before_xyz, before_intensity, n, after, m, p ? p->dist_mode : 0, p ? p->max_distance_squared : 0.f, lambda_geometric, init_T));
    const PoseLoopFields loop{p->eps_rotation, p->eps_translation, p->max_iterations, p->sync_every, p->verbose, "pairs"};
    MI_TRY(pose_check_fields(who, loop));
    if (c->distributed()) { set_error("%s: single-GPU contexts only", who); return MI_ERR_STATE; }
    MI_ENTER(c);
    mi_ctx::ColorBuffers& b = c->color;
    StageClock clock(c, b.ms);         // mi_icp_color_times

    SearchFront f;
    ColorStepArgs a;
    PlaneState h;
    MI_TRY(color_prepare(c, who, clock, before_xyz, before_intensity, n, after, m, p->max_distance_squared, lambda_geometric, init_T, false, &f, &a, &h));

    const int fma = p->dist_mode == MI_DIST_FMA;
    MI_TRY(pose_loop_run(c, b.loop, clock, who, n, loop, &h, [&] { return color_step(f.g, a, fma, c->stream); }));
    return pose_loop_results(clock, h, out_T, iterations, error, stop_reason);
}

extern "C" int mi_color_system(mi_ctx* c, const float* before_xyz, const float* before_intensity, int n, const float* after_xyz, const float* after_normals_xyz,
                               const float* after_intensity, const float* after_gradients_xyz, int m, const float T[16], int dist_mode,
                               float max_distance_squared, float lambda_geometric, double out_sums[32], float out_centre[3], int* out_idx)
{
    const char* who = "mi_color_system";
    if (c && !out_sums) { set_error("%s: null out_sums", who); return MI_ERR_INVALID_ARG; }
    const ColorFixed after{after_xyz, after_normals_xyz, after_intensity, after_gradients_xyz};
    MI_TRY(check_arguments(who, c, before_xyz, before_intensity, n, after, m, dist_mode, max_distance_squared, lambda_geometric, T));
    if (c->distributed()) { set_error("%s: single-GPU contexts only", who); return MI_ERR_STATE; }
    MI_ENTER(c);
    mi_ctx::ColorBuffers& b = c->color;
    StageClock clock(c, b.ms);         // mi_icp_color_times

    SearchFront f;
    ColorStepArgs a;
    PlaneState h;
    MI_TRY(color_prepare(c, who, clock, before_xyz, before_intensity, n, after, m, max_distance_squared, lambda_geometric, T, out_idx != nullptr, &f, &a, &h));

    const int fma = dist_mode == MI_DIST_FMA;
    MI_TRY(pose_loop_system_run(c, b.loop, clock, n, &h, out_idx, [&] { return color_step(f.g, a, fma, c->stream); }));
    return pose_loop_system_finish(c, clock, h, out_sums, out_centre);
}

extern "C" int mi_icp_color_times(mi_ctx* c, double out_ms[MI_COLOR_STAGES]) { return stage_times("mi_icp_color_times", c ? c->color.ms : nullptr, out_ms); }
