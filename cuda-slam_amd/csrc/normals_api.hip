// mi_estimate_normals behind the C ABI: argument checks, the reserves of the call's own buffers in the context, the search front end in
// self mode (search_front.hip: upload, input check and its one read-back, the cell grid over the cloud under mi_knn_search's
// points-per-cell rule, the curve order), the arguments and the fused launch of normals_kernels.hip, and the download of what was asked for.
#include <hip/hip_runtime.h>

#include <cmath>

#include "context.h"

using namespace mislam;

extern "C" int mi_estimate_normals(mi_ctx* c, const float* cloud_xyz, int n, int k, int dist_mode, float max_distance_squared,
                                   const float* viewpoint3, float* normals_xyz, float* curvature, int* count)
{
    if (!c) { set_error("mi_estimate_normals: null context"); return MI_ERR_INVALID_ARG; }
    if (!cloud_xyz || !normals_xyz) { set_error("mi_estimate_normals: null cloud_xyz or normals_xyz"); return MI_ERR_INVALID_ARG; }
    if (n < 1) { set_error("mi_estimate_normals: empty cloud (n = %d)", n); return MI_ERR_INVALID_ARG; }
    if (k < 2 || k > MI_KNN_MAX_K) { set_error("mi_estimate_normals: k = %d outside [2, %d]", k, MI_KNN_MAX_K); return MI_ERR_INVALID_ARG; }
    if (dist_mode != MI_DIST_CPU_ROUNDING && dist_mode != MI_DIST_FMA) { set_error("mi_estimate_normals: bad dist_mode %d", dist_mode); return MI_ERR_INVALID_ARG; }
    if (!(max_distance_squared >= 0.f)) { set_error("mi_estimate_normals: max_distance_squared %g is NaN or negative", (double)max_distance_squared); return MI_ERR_INVALID_ARG; }
    if (viewpoint3 && !(std::isfinite(viewpoint3[0]) && std::isfinite(viewpoint3[1]) && std::isfinite(viewpoint3[2]))) {
        set_error("mi_estimate_normals: non-finite viewpoint (%g, %g, %g)", (double)viewpoint3[0], (double)viewpoint3[1], (double)viewpoint3[2]);
        return MI_ERR_INVALID_ARG;
    }
    if (c->distributed()) { set_error("mi_estimate_normals: single-GPU contexts only"); return MI_ERR_STATE; }
    MI_ENTER(c);
    mi_ctx::NormalsBuffers& b = c->normals;
    StageClock clock(c, b.ms);         // mi_estimate_normals_times

    const size_t np = (size_t)n;
    CallBuffers bufs;
    MI_TRY(search_front_reserve(b.front, np, np, true));
    MI_TRY(bufs.result(b.out_normals, 3 * np, normals_xyz)); MI_TRY(bufs.result(b.out_curvature, np, curvature)); MI_TRY(bufs.result(b.out_count, np, count));
    MI_TRY(clock.mark(0));

    SearchFront f;
    MI_TRY(search_front_upload_and_check(c, b.front, clock, "mi_estimate_normals", cloud_xyz, n, nullptr, n, &f));
    const float ppc = c->tune.knn_points_per_cell > 0.f ? c->tune.knn_points_per_cell : knn_default_points_per_cell(k);   // mi_knn_search's grid, cell size included
    MI_TRY(search_front_index_and_order(c, b.front, clock, "mi_estimate_normals", ppc, &f));

    KnnNormalsArgs a{};
    a.q = search_front_queries(b.front, f);
    a.c = search_front_cloud(b.front);
    a.k = k; a.max_d2 = max_distance_squared;
    a.oriented = viewpoint3 ? 1 : 0;
    for (int i = 0; i < 3; i++) a.view[i] = viewpoint3 ? (double)viewpoint3[i] : 0.0;
    a.normals = b.out_normals.p; a.curvature = curvature ? b.out_curvature.p : nullptr; a.count = count ? b.out_count.p : nullptr;
    // host-side shape checks before the hand-written kernel runs: every array it indexes is as long as the launch assumes
    if (!search_front_fits(b.front, f) || !bufs.fits()) {
        set_error("internal: mi_estimate_normals buffers shorter than the launch");
        return MI_ERR_STATE;
    }
    MI_TRY(search_front_timed_launch(c, b.front, clock, [&] { return knn_normals(f.g, a, dist_mode == MI_DIST_FMA, c->stream); }));

    MI_TRY(bufs.download(c->stream));
    MI_HIP(hipStreamSynchronize(c->stream));
    MI_TRY(clock.mark(6));
    clock.finish();
    return MI_OK;
}

extern "C" int mi_estimate_normals_times(mi_ctx* c, double out_ms[MI_NORMALS_STAGES]) { return stage_times("mi_estimate_normals_times", c ? c->normals.ms : nullptr, out_ms); }
