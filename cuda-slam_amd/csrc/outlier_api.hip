// mi_remove_outliers behind the C ABI: argument checks, the reserves of the call's own buffers in the context, the search front end in
// self mode (search_front.hip: upload, input check and its one read-back, the cell grid over the cloud, the curve order), the method's
// launch of outlier_kernels.hip (the fused search-and-score, or the fixed-radius count), the statistics, the flags, their compaction and the
// download of what was asked for.
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
    CallBuffers bufs;                  // (in the order of the download)
    MI_TRY(search_front_reserve(b.front, np, np, true));
    MI_TRY(bufs.watch(b.front.staging, 3 * np));                                   // the front end's; what the compaction gathers from
    MI_TRY(bufs.need(b.ostate, 1));
    MI_TRY(bufs.need(b.keep, np, keep)); MI_TRY(bufs.need(b.tile_counts, (size_t)tiles));
    if (statistical) { MI_TRY(bufs.need(b.score, np)); MI_TRY(bufs.need(b.partials, (size_t)stat_blocks)); MI_TRY(bufs.result(b.out_mean, np, mean_distance)); }
    if (!statistical || neighbours) MI_TRY(bufs.need(b.count, np, neighbours));
    if (out_xyz) MI_TRY(bufs.need(b.out_xyz, 3 * np));                            // (their rows go once their number is known)
    if (out_index) MI_TRY(bufs.need(b.out_index, np));
    MI_TRY(clock.mark(0));

    SearchFront f;
    MI_TRY(search_front_upload_and_check(c, b.front, clock, "mi_remove_outliers", cloud_xyz, n, nullptr, n, &f));
    // the cell grid over the cloud: mi_knn_search's for the statistical method, cell size included; a cell about a radius long for the other
    const float ppc = c->tune.knn_points_per_cell > 0.f ? c->tune.knn_points_per_cell
                      : (statistical ? knn_default_points_per_cell(k) : radius_points_per_cell(f.bbox, n, p->radius, c->tune.outlier_radius_cell));
    MI_TRY(search_front_index_and_order(c, b.front, clock, "mi_remove_outliers", ppc, &f));

    // host-side shape checks before the hand-written kernels run: every array they index is as long as the launches assume
    if (!search_front_fits(b.front, f) || !bufs.fits()) {
        set_error("internal: mi_remove_outliers buffers shorter than the launch");
        return MI_ERR_STATE;
    }
    const int fma = p->dist_mode == MI_DIST_FMA;
    MI_TRY(search_front_timed_launch(c, b.front, clock, [&] {
        if (statistical) {
            KnnOutlierArgs a{};
            a.q = search_front_queries(b.front, f);
            a.k = k;
            a.score = b.score.p; a.count = neighbours ? b.count.p : nullptr;
            return knn_outlier_score(f.g, a, fma, c->stream);
        }
        RadiusCountArgs a{};
        a.q = search_front_queries(b.front, f);
        a.r2 = r2; a.min_neighbours = min_nb;
        a.count = b.count.p;
        return radius_count(f.g, a, fma, neighbours ? 0 : 1, c->stream);
    }));

    if (statistical) {
        MI_HIP(outlier_statistics(b.score.p, n, p->std_ratio, b.partials.p, b.ostate.p, c->stream));
        MI_HIP(outlier_flags_statistical(b.score.p, n, b.ostate.p, b.keep.p, mean_distance ? b.out_mean.p : nullptr, c->stream));
    } else {
        MI_HIP(hipMemsetAsync(b.ostate.p, 0, sizeof(OutlierState), c->stream));    // (mean, stddev, threshold: the host states them below)
        MI_HIP(outlier_flags_radius(b.count.p, n, min_nb, b.keep.p, c->stream));
    }
    MI_TRY(compact_enqueue(c, b.front, b.keep.p, n, b.tile_counts.p, out_index ? b.out_index.p : nullptr, out_xyz ? b.out_xyz.p : nullptr, b.ostate.p));

    // the state once, with the per-point results; then the kept rows, whose number the state has brought
    MI_TRY(compact_read_state(c, b.ostate.p, 1));
    MI_TRY(bufs.download(c->stream));
    MI_HIP(hipStreamSynchronize(c->stream));
    const OutlierState* os = compact_host_state(c);
    long long kept;
    if (!compact_kept(c, 0, n, &kept)) { set_error("internal: mi_remove_outliers kept %lld of %d points", kept, n); return MI_ERR_STATE; }
    if (stats) {
        *stats = mi_outlier_stats{};
        stats->mean = statistical ? os->mean : 0.0;
        stats->stddev = statistical ? os->stddev : 0.0;
        stats->threshold = statistical ? os->threshold : (double)min_nb;
        stats->kept = kept;
    }
    MI_TRY(compact_download(c, kept, out_xyz, b.out_xyz.p, out_index, b.out_index.p));
    *out_n = (int)kept;
    MI_TRY(clock.mark(6));
    clock.finish();
    return MI_OK;
}

extern "C" int mi_remove_outliers_times(mi_ctx* c, double out_ms[MI_OUTLIER_STAGES]) { return stage_times("mi_remove_outliers_times", c ? c->outlier.ms : nullptr, out_ms); }
