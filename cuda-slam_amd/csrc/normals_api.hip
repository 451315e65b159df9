// mi_estimate_normals behind the C ABI: argument checks, the call's own buffers in the context, the upload, then mi_knn_search's
// stages in self mode through the same helpers -- the input check and its one read-back (knn_check_inputs), the cell grid over the
// cloud under the same points-per-cell rule (grid_reserve / grid_build_into), the curve order (morton_order / permute_soa) -- the
// fused launch of normals_kernels.hip, and the download of what was asked for.
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
    MI_TRY(b.staging.reserve(3 * np));
    MI_TRY(b.cx.reserve(np)); MI_TRY(b.cy.reserve(np)); MI_TRY(b.cz.reserve(np));
    MI_TRY(b.qx.reserve(np)); MI_TRY(b.qy.reserve(np)); MI_TRY(b.qz.reserve(np));
    MI_TRY(b.range_lo_hi.reserve(2 * 6 * KNN_RANGE_BLOCKS)); MI_TRY(b.range_bad.reserve(2 * KNN_RANGE_BLOCKS)); MI_TRY(b.state.reserve(1));
    MI_TRY(b.order.reserve(np));
    MI_TRY(b.out_normals.reserve(3 * np));
    if (curvature) MI_TRY(b.out_curvature.reserve(np));
    if (count) MI_TRY(b.out_count.reserve(np));
    MI_TRY(clock.mark(0));

    MI_TRY(host_to_device(c, b.staging.p, cloud_xyz, sizeof(float) * 3 * np));
    MI_HIP(aos_to_soa(b.staging.p, n, n, b.cx.p, b.cy.p, b.cz.p, nullptr, c->stream));
    MI_TRY(clock.mark(1));

    MI_HIP(knn_check_inputs(b.cx.p, b.cy.p, b.cz.p, n, nullptr, nullptr, nullptr, n, b.range_lo_hi.p, b.range_bad.p, b.state.p, c->stream));
    KnnState* st = reinterpret_cast<KnnState*>(c->h_scratch);     // (pinned, 256 bytes)
    static_assert(sizeof(KnnState) <= 64 * sizeof(float), "KnnState must fit the context's pinned scratch");
    MI_HIP(hipMemcpyAsync(st, b.state.p, sizeof(KnnState), hipMemcpyDeviceToHost, c->stream));
    MI_HIP(hipStreamSynchronize(c->stream));
    MI_TRY(clock.mark(2));
    // everything that can refuse the input is known here, before any output array has been touched
    if (st->bad_cloud != KNN_NO_POINT) {
        set_error("mi_estimate_normals: cloud_xyz point %d has a non-finite coordinate or one above 1e18 in magnitude", st->bad_cloud);
        return MI_ERR_INVALID_ARG;
    }

    // the cell grid over the cloud: mi_knn_search's, cell size included
    const float bbox[6] = {st->lo[0], st->lo[1], st->lo[2], st->hi[0], st->hi[1], st->hi[2]};
    const float ppc = c->tune.knn_points_per_cell > 0.f ? c->tune.knn_points_per_cell : knn_default_points_per_cell(k);
    NnGridView g{};
    MI_TRY(grid_reserve(b.cells, bbox, n, 0, ppc, &g));
    MI_TRY(clock.mark(0));
    if (g.nx < 1 || g.ny < 1 || g.nz < 1 || g.nx > GRID_MAX_DIM || g.ny > GRID_MAX_DIM || g.nz > GRID_MAX_DIM || !(g.inv_h > 0.f) || !(g.h_lo > 0.f)) {
        set_error("internal: mi_estimate_normals planned a %d x %d x %d grid", g.nx, g.ny, g.nz);
        return MI_ERR_STATE;
    }
    const size_t n_cells = (size_t)g.nx * g.ny * g.nz;
    MI_TRY(grid_build_into(b.cells, g, b.cx.p, b.cy.p, b.cz.p, n, c->stream));
    MI_TRY(clock.mark(3));

    // the cloud along its curve: order[s] = the caller's index of sorted slot s
    MortonArgs ma{};
    MI_TRY(morton_args(b.morton, b.cx.p, b.cy.p, b.cz.p, n, b.order.p, &ma));
    MI_HIP(morton_order(ma, c->stream));
    MI_HIP(permute_soa(b.cx.p, b.cy.p, b.cz.p, b.order.p, n, n, b.qx.p, b.qy.p, b.qz.p, c->stream));
    MI_TRY(clock.mark(4));

    KnnNormalsArgs a{};
    a.qx = b.qx.p; a.qy = b.qy.p; a.qz = b.qz.p; a.order = b.order.p;
    a.cx = b.cx.p; a.cy = b.cy.p; a.cz = b.cz.p;
    a.n = n; a.k = k; a.max_d2 = max_distance_squared;
    for (int i = 0; i < 3; i++) a.hi[i] = bbox[3 + i];
    a.oriented = viewpoint3 ? 1 : 0;
    for (int i = 0; i < 3; i++) a.view[i] = viewpoint3 ? (double)viewpoint3[i] : 0.0;
    a.normals = b.out_normals.p; a.curvature = curvature ? b.out_curvature.p : nullptr; a.count = count ? b.out_count.p : nullptr;
    // host-side shape checks before the hand-written kernel runs: every array it indexes is as long as the launch assumes
    if (b.qx.cap < np || b.qy.cap < np || b.qz.cap < np || b.cx.cap < np || b.cy.cap < np || b.cz.cap < np || b.order.cap < np ||
        b.out_normals.cap < 3 * np || (curvature && b.out_curvature.cap < np) || (count && b.out_count.cap < np) ||
        b.cells.start.cap < n_cells + 1 || b.cells.pts.cap < np) {
        set_error("internal: mi_estimate_normals buffers shorter than the launch");
        return MI_ERR_STATE;
    }
    const bool timed = c->prof.on;
    if (timed) {
        for (hipEvent_t& e : b.ev)
            if (!e) MI_HIP(hipEventCreate(&e));
        MI_HIP(hipEventRecord(b.ev[0], c->stream));
    }
    MI_HIP(knn_normals(g, a, dist_mode == MI_DIST_FMA, c->stream));
    if (timed) MI_HIP(hipEventRecord(b.ev[1], c->stream));
    MI_TRY(clock.mark(5));
    if (timed) {
        float ms = 0.f;
        MI_HIP(hipEventElapsedTime(&ms, b.ev[0], b.ev[1]));
        b.ms[5] = (double)ms;
    }

    MI_HIP(hipMemcpyAsync(normals_xyz, b.out_normals.p, sizeof(float) * 3 * np, hipMemcpyDeviceToHost, c->stream));
    if (curvature) MI_HIP(hipMemcpyAsync(curvature, b.out_curvature.p, sizeof(float) * np, hipMemcpyDeviceToHost, c->stream));
    if (count) MI_HIP(hipMemcpyAsync(count, b.out_count.p, sizeof(int) * np, hipMemcpyDeviceToHost, c->stream));
    MI_HIP(hipStreamSynchronize(c->stream));
    MI_TRY(clock.mark(6));
    clock.finish();
    return MI_OK;
}

extern "C" int mi_estimate_normals_times(mi_ctx* c, double out_ms[MI_NORMALS_STAGES])
{
    if (!c || !out_ms) { set_error("mi_estimate_normals_times: null argument"); return MI_ERR_INVALID_ARG; }
    for (int i = 0; i < MI_NORMALS_STAGES; i++) out_ms[i] = c->normals.ms[i];
    return MI_OK;
}
