// mi_icp_plane_register and mi_plane_system behind the C ABI, up to the step kernel's arguments: argument checks, the reserves of the call's
// own buffers in the context, the normals' upload and input check, the search front end with the fixed cloud as the cloud and the moving cloud
// as the queries (search_front.hip: uploads, input check and its one read-back, the cell grid over the fixed cloud under mi_knn_search's
// points-per-cell rule for k = 1, the curve order of the moving cloud).  The state block, the iterations of plane_kernels.hip in batches of
// sync_every between host reads of the state, and the results are the pose loop's (pose_loop.hip), which gets the step's launch.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "context.h"

using namespace mislam;

extern "C" void mi_plane_params_default(mi_plane_params* p)
{
    if (!p) return;
    std::memset(p, 0, sizeof *p);
    p->eps_rotation = 1e-6f;
    p->eps_translation = 1e-6f;
    p->max_iterations = 50;
    p->max_distance_squared = INFINITY;
    p->dist_mode = MI_DIST_CPU_ROUNDING;
    p->sync_every = 0;
}

namespace {

// what both entry points refuse alike, before the context is touched
int check_arguments(const char* who, mi_ctx* c, const float* before_xyz, int n, const float* after_xyz, const float* normals_xyz, int m, int dist_mode,
                    float max_d2, const float* T)
{
    if (!c) { set_error("%s: null context", who); return MI_ERR_INVALID_ARG; }
    if (!before_xyz || !after_xyz || !normals_xyz) { set_error("%s: null before_xyz, after_xyz or after_normals_xyz", who); return MI_ERR_INVALID_ARG; }
    if (n < 1 || m < 1) { set_error("%s: empty moving or fixed cloud (n = %d, m = %d)", who, n, m); return MI_ERR_INVALID_ARG; }
    if (dist_mode != MI_DIST_CPU_ROUNDING && dist_mode != MI_DIST_FMA) { set_error("%s: bad dist_mode %d", who, dist_mode); return MI_ERR_INVALID_ARG; }
    if (!(max_d2 >= 0.f)) { set_error("%s: max_distance_squared %g is NaN or negative", who, (double)max_d2); return MI_ERR_INVALID_ARG; }
    return pose_check_transform(who, T);
}

// Stages 0 - 4 of either call and the state block at pose T: after it the step kernel's arguments are complete and checked against the buffers.
int plane_prepare(mi_ctx* c, const char* who, StageClock& clock, const float* before_xyz, int n, const float* after_xyz, const float* normals_xyz, int m,
                  float max_d2, const float* T, bool want_idx, SearchFront* f, PlaneStepArgs* a, PlaneState* h)
{
    mi_ctx::PlaneBuffers& b = c->plane;
    const size_t np = (size_t)n, mp = (size_t)m;
    CallBuffers bufs;
    MI_TRY(search_front_reserve(b.front, np, mp, false));
    MI_TRY(bufs.need(b.nx, mp)); MI_TRY(bufs.need(b.ny, mp)); MI_TRY(bufs.need(b.nz, mp)); MI_TRY(bufs.need(b.normals, mp)); MI_TRY(bufs.need(b.nstate, 1));
    MI_TRY(pose_loop_reserve(b.loop, n, want_idx));
    MI_TRY(clock.mark(0));

    MI_TRY(search_front_enqueue_normals(c, b.front, normals_xyz, m, b.nx.p, b.ny.p, b.nz.p, b.normals.p, b.nstate.p));
    MI_TRY(search_front_upload_and_check(c, b.front, clock, who, after_xyz, m, before_xyz, n, f, "after_xyz", "before_xyz"));
    MI_TRY(search_front_refuse_normals(c, clock, who, "after_normals_xyz", b.nstate.p));
    const float ppc = c->tune.knn_points_per_cell > 0.f ? c->tune.knn_points_per_cell : knn_default_points_per_cell(1);   // mi_knn_search's grid for k = 1
    MI_TRY(search_front_index_and_order(c, b.front, clock, who, ppc, f));

    float centre[3];
    for (int i = 0; i < 3; i++) centre[i] = 0.5f * (f->bbox[i] + f->bbox[3 + i]);
    MI_TRY(pose_loop_upload_state(c, b.loop, clock, T, centre, h));

    *a = PlaneStepArgs{};
    a->state = b.loop.state.p;
    a->q = search_front_queries(b.front, *f);
    a->c = search_front_cloud(b.front);
    a->normals = b.normals.p;
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

extern "C" int mi_icp_plane_register(mi_ctx* c, const float* before_xyz, int n, const float* after_xyz, const float* after_normals_xyz, int m,
                                     const mi_plane_params* p, const float init_T[16], float out_T[16], int* iterations, float* error, int* stop_reason)
{
    const char* who = "mi_icp_plane_register";
    if (c && (!p || !out_T)) { set_error("%s: null params or out_T", who); return MI_ERR_INVALID_ARG; }
    MI_TRY(check_arguments(who, c, before_xyz, n, after_xyz, after_normals_xyz, m, p ? p->dist_mode : 0, p ? p->max_distance_squared : 0.f, init_T));
    const PoseLoopFields loop{p->eps_rotation, p->eps_translation, p->max_iterations, p->sync_every, p->verbose, "pairs"};
    MI_TRY(pose_check_fields(who, loop));
    if (c->distributed()) { set_error("%s: single-GPU contexts only", who); return MI_ERR_STATE; }
    MI_ENTER(c);
    mi_ctx::PlaneBuffers& b = c->plane;
    StageClock clock(c, b.ms);         // mi_icp_plane_times

    SearchFront f;
    PlaneStepArgs a;
    PlaneState h;
    MI_TRY(plane_prepare(c, who, clock, before_xyz, n, after_xyz, after_normals_xyz, m, p->max_distance_squared, init_T, false, &f, &a, &h));

    const int fma = p->dist_mode == MI_DIST_FMA;
    MI_TRY(pose_loop_run(c, b.loop, clock, who, n, loop, &h, [&] { return plane_step(f.g, a, fma, c->stream); }));
    return pose_loop_results(clock, h, out_T, iterations, error, stop_reason);
}

extern "C" int mi_plane_system(mi_ctx* c, const float* before_xyz, int n, const float* after_xyz, const float* after_normals_xyz, int m, const float T[16],
                               int dist_mode, float max_distance_squared, double out_sums[32], float out_centre[3], int* out_idx)
{
    const char* who = "mi_plane_system";
    if (c && !out_sums) { set_error("%s: null out_sums", who); return MI_ERR_INVALID_ARG; }
    MI_TRY(check_arguments(who, c, before_xyz, n, after_xyz, after_normals_xyz, m, dist_mode, max_distance_squared, T));
    if (c->distributed()) { set_error("%s: single-GPU contexts only", who); return MI_ERR_STATE; }
    MI_ENTER(c);
    mi_ctx::PlaneBuffers& b = c->plane;
    StageClock clock(c, b.ms);         // mi_icp_plane_times

    SearchFront f;
    PlaneStepArgs a;
    PlaneState h;
    MI_TRY(plane_prepare(c, who, clock, before_xyz, n, after_xyz, after_normals_xyz, m, max_distance_squared, T, out_idx != nullptr, &f, &a, &h));

    const int fma = dist_mode == MI_DIST_FMA;
    MI_TRY(pose_loop_system_run(c, b.loop, clock, n, &h, out_idx, [&] { return plane_step(f.g, a, fma, c->stream); }));
    return pose_loop_system_finish(c, clock, h, out_sums, out_centre);
}

extern "C" int mi_icp_plane_times(mi_ctx* c, double out_ms[MI_PLANE_STAGES]) { return stage_times("mi_icp_plane_times", c ? c->plane.ms : nullptr, out_ms); }
