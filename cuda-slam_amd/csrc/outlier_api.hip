// mi_remove_outliers behind the C ABI: argument checks, the call's own buffers in the context, the upload, then mi_estimate_normals'
// stages through the same helpers -- the input check and its one read-back (knn_check_inputs), the cell grid over the cloud
// (grid_reserve / grid_build_into), the curve order (morton_order / permute_soa) -- the method's launch of outlier_kernels.hip (the fused
// search-and-score, or the fixed-radius count), the statistics, the flags, their compaction and the download of what was asked for.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "context.h"

using namespace mislam;

extern "C" void mi_outlier_params_default(mi_outlier_params* p)
{
    if (!p) return;
    *p = mi_outlier_params{};
    p->method = MI_OUTLIER_STATISTICAL;
    p->dist_mode = MI_DIST_CPU_ROUNDING;
    p->k = 16;
    p->std_ratio = 2.0f;
    p->radius = 0.0f;
    p->min_neighbours = 1;
}

// Points per cell of the radius method's grid: the number that makes a cell's edge `cell_in_radii` radii long (1 unless
// MISLAM_OUTLIER_RADIUS_CELL says otherwise), so that a ball reaches into the 27 cells around its point's and rarely further.  An axis
// shorter than that edge is one layer of cells.  Bounded below by the k-NN rule's floor (at most one cell per point: a small radius in a
// sparse cloud must not buy more cells than points) and above by n (one cell); grid_plan keeps the counts within GRID_MAX_DIM.
// A rule by reasoning, not by measurement.
static float radius_points_per_cell(const float bbox[6], int n, float radius, float cell_in_radii)
{
    const double edge = (double)cell_in_radii * (double)radius;
    double cells = 1.0;
    for (int a = 0; a < 3; a++) {
        const double ext = (double)bbox[3 + a] - (double)bbox[a];
        if (ext > edge) cells *= ext / edge;
    }
    const double ppc = (double)n / cells;                                          // (cells >= 1, possibly +inf: ppc in [0, n])
    return (float)std::min(std::max(ppc, (double)knn_default_points_per_cell(1)), (double)n);
}

extern "C" int mi_remove_outliers(mi_ctx* c, const float* cloud_xyz, int n, const mi_outlier_params* p, float* out_xyz, int* out_index, int* out_n,
                                  unsigned char* keep, float* mean_distance, int* neighbours, mi_outlier_stats* stats)
{
    if (!c) { set_error("mi_remove_outliers: null context"); return MI_ERR_INVALID_ARG; }
    if (!cloud_xyz || !p || !out_n) { set_error("mi_remove_outliers: null cloud_xyz, params or out_n"); return MI_ERR_INVALID_ARG; }
    if (n < 1) { set_error("mi_remove_outliers: empty cloud (n = %d)", n); return MI_ERR_INVALID_ARG; }
    if (p->method != MI_OUTLIER_STATISTICAL && p->method != MI_OUTLIER_RADIUS) { set_error("mi_remove_outliers: bad method %d", p->method); return MI_ERR_INVALID_ARG; }
    if (p->dist_mode != MI_DIST_CPU_ROUNDING && p->dist_mode != MI_DIST_FMA) { set_error("mi_remove_outliers: bad dist_mode %d", p->dist_mode); return MI_ERR_INVALID_ARG; }
    const bool statistical = p->method == MI_OUTLIER_STATISTICAL;
    const int k = p->k, min_nb = p->min_neighbours;
    const float r2 = p->radius * p->radius;                                        // one IEEE fp32 multiplication (-ffp-contract=off)
    if (statistical) {
        if (k < 1 || k > MI_KNN_MAX_K) { set_error("mi_remove_outliers: k = %d outside [1, %d]", k, MI_KNN_MAX_K); return MI_ERR_INVALID_ARG; }
        if (!(std::isfinite(p->std_ratio) && p->std_ratio >= 0.f)) { set_error("mi_remove_outliers: std_ratio %g is NaN, infinite or negative", (double)p->std_ratio); return MI_ERR_INVALID_ARG; }
    } else {
        if (!(std::isfinite(p->radius) && p->radius > 0.f)) { set_error("mi_remove_outliers: radius %g is NaN, infinite or not positive", (double)p->radius); return MI_ERR_INVALID_ARG; }
        if (!std::isfinite(r2)) { set_error("mi_remove_outliers: the square of radius %g is not finite", (double)p->radius); return MI_ERR_INVALID_ARG; }
        if (min_nb < 1) { set_error("mi_remove_outliers: min_neighbours = %d below 1", min_nb); return MI_ERR_INVALID_ARG; }
    }
    if (c->distributed()) { set_error("mi_remove_outliers: single-GPU contexts only"); return MI_ERR_STATE; }
    MI_ENTER(c);
    mi_ctx::OutlierBuffers& b = c->outlier;
    StageClock clock(c, b.ms);         // mi_remove_outliers_times

    const size_t np = (size_t)n;
    const int tiles = outlier_scan_tiles(n), stat_blocks = outlier_stat_blocks(n);
    MI_TRY(b.staging.reserve(3 * np));
    MI_TRY(b.cx.reserve(np)); MI_TRY(b.cy.reserve(np)); MI_TRY(b.cz.reserve(np));
    MI_TRY(b.qx.reserve(np)); MI_TRY(b.qy.reserve(np)); MI_TRY(b.qz.reserve(np));
    MI_TRY(b.range_lo_hi.reserve(2 * 6 * KNN_RANGE_BLOCKS)); MI_TRY(b.range_bad.reserve(2 * KNN_RANGE_BLOCKS)); MI_TRY(b.state.reserve(1)); MI_TRY(b.ostate.reserve(1));
    MI_TRY(b.order.reserve(np));
    MI_TRY(b.keep.reserve(np)); MI_TRY(b.tile_counts.reserve((size_t)tiles));
    if (statistical) { MI_TRY(b.score.reserve(np)); MI_TRY(b.partials.reserve((size_t)stat_blocks)); }
    if (!statistical || neighbours) MI_TRY(b.count.reserve(np));
    if (statistical && mean_distance) MI_TRY(b.out_mean.reserve(np));
    if (out_xyz) MI_TRY(b.out_xyz.reserve(3 * np));
    if (out_index) MI_TRY(b.out_index.reserve(np));
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
    // everything that can refuse the input is known here, before any output has been touched
    if (st->bad_cloud != KNN_NO_POINT) {
        set_error("mi_remove_outliers: cloud_xyz point %d has a non-finite coordinate or one above 1e18 in magnitude", st->bad_cloud);
        return MI_ERR_INVALID_ARG;
    }

    // the cell grid over the cloud: mi_knn_search's for the statistical method, cell size included; a cell about a radius long for the other
    const float bbox[6] = {st->lo[0], st->lo[1], st->lo[2], st->hi[0], st->hi[1], st->hi[2]};
    const float ppc = c->tune.knn_points_per_cell > 0.f ? c->tune.knn_points_per_cell
                      : (statistical ? knn_default_points_per_cell(k) : radius_points_per_cell(bbox, n, p->radius, c->tune.outlier_radius_cell));
    NnGridView g{};
    MI_TRY(grid_reserve(b.cells, bbox, n, 0, ppc, &g));
    MI_TRY(clock.mark(0));
    if (g.nx < 1 || g.ny < 1 || g.nz < 1 || g.nx > GRID_MAX_DIM || g.ny > GRID_MAX_DIM || g.nz > GRID_MAX_DIM || !(g.inv_h > 0.f) || !(g.h_lo > 0.f)) {
        set_error("internal: mi_remove_outliers planned a %d x %d x %d grid", g.nx, g.ny, g.nz);
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

    // host-side shape checks before the hand-written kernels run: every array they index is as long as the launches assume
    if (b.qx.cap < np || b.qy.cap < np || b.qz.cap < np || b.order.cap < np || b.staging.cap < 3 * np || b.keep.cap < np || b.tile_counts.cap < (size_t)tiles ||
        (statistical && (b.score.cap < np || b.partials.cap < (size_t)stat_blocks)) || ((!statistical || neighbours) && b.count.cap < np) ||
        (statistical && mean_distance && b.out_mean.cap < np) || (out_xyz && b.out_xyz.cap < 3 * np) || (out_index && b.out_index.cap < np) ||
        b.cells.start.cap < n_cells + 1 || b.cells.pts.cap < np) {
        set_error("internal: mi_remove_outliers buffers shorter than the launch");
        return MI_ERR_STATE;
    }
    const bool timed = c->prof.on;
    if (timed) {
        for (hipEvent_t& e : b.ev)
            if (!e) MI_HIP(hipEventCreate(&e));
        MI_HIP(hipEventRecord(b.ev[0], c->stream));
    }
    const int fma = p->dist_mode == MI_DIST_FMA;
    if (statistical) {
        KnnOutlierArgs a{};
        a.qx = b.qx.p; a.qy = b.qy.p; a.qz = b.qz.p; a.order = b.order.p;
        a.n = n; a.k = k;
        for (int i = 0; i < 3; i++) a.hi[i] = bbox[3 + i];
        a.score = b.score.p; a.count = neighbours ? b.count.p : nullptr;
        MI_HIP(knn_outlier_score(g, a, fma, c->stream));
    } else {
        RadiusCountArgs a{};
        a.qx = b.qx.p; a.qy = b.qy.p; a.qz = b.qz.p; a.order = b.order.p;
        a.n = n; a.r2 = r2; a.min_neighbours = min_nb;
        for (int i = 0; i < 3; i++) a.hi[i] = bbox[3 + i];
        a.count = b.count.p;
        MI_HIP(radius_count(g, a, fma, neighbours ? 0 : 1, c->stream));
    }
    if (timed) MI_HIP(hipEventRecord(b.ev[1], c->stream));
    MI_TRY(clock.mark(5));
    if (timed) {
        float ms = 0.f;
        MI_HIP(hipEventElapsedTime(&ms, b.ev[0], b.ev[1]));
        b.ms[5] = (double)ms;
    }

    if (statistical) {
        MI_HIP(outlier_statistics(b.score.p, n, p->std_ratio, b.partials.p, b.ostate.p, c->stream));
        MI_HIP(outlier_flags_statistical(b.score.p, n, b.ostate.p, b.keep.p, mean_distance ? b.out_mean.p : nullptr, c->stream));
    } else {
        MI_HIP(hipMemsetAsync(b.ostate.p, 0, sizeof(OutlierState), c->stream));    // (mean, stddev, threshold: the host states them below)
        MI_HIP(outlier_flags_radius(b.count.p, n, min_nb, b.keep.p, c->stream));
    }
    OutlierCompactArgs ca{};
    ca.keep = b.keep.p; ca.xyz = b.staging.p; ca.n = n; ca.tile_counts = b.tile_counts.p;
    ca.out_index = out_index ? b.out_index.p : nullptr; ca.out_xyz = out_xyz ? b.out_xyz.p : nullptr; ca.state = b.ostate.p;
    MI_HIP(outlier_compact(ca, c->stream));

    // the state once, with the per-point results; then the kept rows, whose number the state has brought
    OutlierState* os = reinterpret_cast<OutlierState*>(c->h_scratch);
    static_assert(sizeof(OutlierState) <= 64 * sizeof(float), "OutlierState must fit the context's pinned scratch");
    MI_HIP(hipMemcpyAsync(os, b.ostate.p, sizeof(OutlierState), hipMemcpyDeviceToHost, c->stream));
    if (keep) MI_HIP(hipMemcpyAsync(keep, b.keep.p, np, hipMemcpyDeviceToHost, c->stream));
    if (statistical && mean_distance) MI_HIP(hipMemcpyAsync(mean_distance, b.out_mean.p, sizeof(float) * np, hipMemcpyDeviceToHost, c->stream));
    if (neighbours) MI_HIP(hipMemcpyAsync(neighbours, b.count.p, sizeof(int) * np, hipMemcpyDeviceToHost, c->stream));
    MI_HIP(hipStreamSynchronize(c->stream));
    const long long kept = os->kept;
    if (kept < 0 || kept > (long long)n) { set_error("internal: mi_remove_outliers kept %lld of %d points", kept, n); return MI_ERR_STATE; }
    if (stats) {
        *stats = mi_outlier_stats{};
        stats->mean = statistical ? os->mean : 0.0;
        stats->stddev = statistical ? os->stddev : 0.0;
        stats->threshold = statistical ? os->threshold : (double)min_nb;
        stats->kept = kept;
    }
    if (kept > 0) {
        if (out_xyz) MI_HIP(hipMemcpyAsync(out_xyz, b.out_xyz.p, sizeof(float) * 3 * (size_t)kept, hipMemcpyDeviceToHost, c->stream));
        if (out_index) MI_HIP(hipMemcpyAsync(out_index, b.out_index.p, sizeof(int) * (size_t)kept, hipMemcpyDeviceToHost, c->stream));
        if (out_xyz || out_index) MI_HIP(hipStreamSynchronize(c->stream));
    }
    *out_n = (int)kept;
    MI_TRY(clock.mark(6));
    clock.finish();
    return MI_OK;
}

extern "C" int mi_remove_outliers_times(mi_ctx* c, double out_ms[MI_OUTLIER_STAGES])
{
    if (!c || !out_ms) { set_error("mi_remove_outliers_times: null argument"); return MI_ERR_INVALID_ARG; }
    for (int i = 0; i < MI_OUTLIER_STAGES; i++) out_ms[i] = c->outlier.ms[i];
    return MI_OK;
}
