// mi_cluster_dbscan behind the C ABI: argument checks, the reserves of the call's own buffers in the context, the search front end in
// self mode (search_front.hip: upload, input check and its one read-back, ONE cell grid over the cloud with cells about one radius long,
// the curve order), the core count (K15's early radius count), K34 - K38 of cluster_kernels.hip over that grid with K15's compaction
// (outlier_compact) between them, one read-back of the two counts, the grouping's sort (radix_sort.hip) where it was asked for, and the
// download of what was asked for.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "context.h"

using namespace mislam;

extern "C" void mi_cluster_params_default(mi_cluster_params* p)
{
    if (!p) return;
    *p = mi_cluster_params{};
    p->radius = 0.0f;
    p->min_points = 1;
    p->min_cluster_size = 1;
    p->max_cluster_size = 0;
    p->dist_mode = MI_DIST_CPU_ROUNDING;
}
static_assert(sizeof(mi_cluster_params) == 64, "mi_cluster_params is 64 bytes (mi_slam.h)");

extern "C" int mi_cluster_dbscan(mi_ctx* c, const float* cloud_xyz, int n, const mi_cluster_params* p, int* labels, int* n_clusters, int* cluster_sizes,
                                 int cluster_cap, unsigned char* is_core, int* grouped_index, int* n_grouped)
{
    if (!c) { set_error("mi_cluster_dbscan: null context"); return MI_ERR_INVALID_ARG; }
    if (!cloud_xyz || !p || !labels || !n_clusters) { set_error("mi_cluster_dbscan: null cloud_xyz, params, labels or n_clusters"); return MI_ERR_INVALID_ARG; }
    if (n < 1) { set_error("mi_cluster_dbscan: empty cloud (n = %d)", n); return MI_ERR_INVALID_ARG; }
    if (p->dist_mode != MI_DIST_CPU_ROUNDING && p->dist_mode != MI_DIST_FMA) { set_error("mi_cluster_dbscan: bad dist_mode %d", p->dist_mode); return MI_ERR_INVALID_ARG; }
    const float r2 = p->radius * p->radius;                                        // one IEEE fp32 multiplication (-ffp-contract=off)
    if (!(std::isfinite(p->radius) && p->radius > 0.f)) { set_error("mi_cluster_dbscan: radius %g is NaN, infinite or not positive", (double)p->radius); return MI_ERR_INVALID_ARG; }
    if (!std::isfinite(r2)) { set_error("mi_cluster_dbscan: the square of radius %g is not finite", (double)p->radius); return MI_ERR_INVALID_ARG; }
    const int min_points = p->min_points, min_size = p->min_cluster_size, max_size = p->max_cluster_size;
    if (min_points < 1) { set_error("mi_cluster_dbscan: min_points = %d below 1", min_points); return MI_ERR_INVALID_ARG; }
    if (min_size < 1) { set_error("mi_cluster_dbscan: min_cluster_size = %d below 1", min_size); return MI_ERR_INVALID_ARG; }
    if (max_size < 0) { set_error("mi_cluster_dbscan: max_cluster_size = %d below 0", max_size); return MI_ERR_INVALID_ARG; }
    if (max_size != 0 && max_size < min_size) { set_error("mi_cluster_dbscan: max_cluster_size = %d below min_cluster_size = %d", max_size, min_size); return MI_ERR_INVALID_ARG; }
    if (cluster_sizes && cluster_cap < 1) { set_error("mi_cluster_dbscan: cluster_sizes given with cluster_cap = %d below 1", cluster_cap); return MI_ERR_INVALID_ARG; }
    if (grouped_index && !n_grouped) { set_error("mi_cluster_dbscan: grouped_index given without n_grouped"); return MI_ERR_INVALID_ARG; }
    if (c->distributed()) { set_error("mi_cluster_dbscan: single-GPU contexts only"); return MI_ERR_STATE; }
    MI_ENTER(c);
    mi_ctx::ClusterBuffers& b = c->cluster;
    // the front end books its stages as every search call's (context.h); t[8] is the core count, t[9] what follows K35: regrouped into
    // the eight slots of mi_cluster_dbscan_times at the end
    double t[10] = {0};
    StageClock clock(c, t);

    const size_t np = (size_t)n;
    const int tiles = outlier_scan_tiles(n);
    const bool counted = min_points > 1;                                           // min_points = 1: every point is core, nothing to count
    const int sizes_cap = cluster_sizes ? std::min(cluster_cap, n) : 0;
    CallBuffers bufs;                  // (cluster_sizes and grouped_index go once their lengths are known)
    MI_TRY(search_front_reserve(b.front, np, np, true));
    MI_TRY(bufs.need(b.ostate, 2));
    if (counted) MI_TRY(bufs.need(b.count, np));
    MI_TRY(bufs.need(b.parent, np)); MI_TRY(bufs.need(b.root_of, np)); MI_TRY(bufs.need(b.size, np)); MI_TRY(bufs.need(b.rank, np)); MI_TRY(bufs.need(b.roots, np));
    MI_TRY(bufs.need(b.labels, np, labels)); MI_TRY(bufs.need(b.keep, np)); MI_TRY(bufs.need(b.core, np, is_core)); MI_TRY(bufs.need(b.tile_counts, (size_t)tiles));
    if (cluster_sizes) MI_TRY(bufs.need(b.sizes_out, (size_t)sizes_cap));
    if (n_grouped) MI_TRY(bufs.need(b.labelled, np));
    if (grouped_index) {
        MI_TRY(bufs.need(b.keys_a, np)); MI_TRY(bufs.need(b.keys_b, np)); MI_TRY(bufs.need(b.group_a, np)); MI_TRY(bufs.need(b.group_b, np));
        MI_TRY(bufs.need(b.sort_temp, radix_sort_temp_bytes(n) + 16));
    }
    MI_TRY(clock.mark(0));

    SearchFront f;
    MI_TRY(search_front_upload_and_check(c, b.front, clock, "mi_cluster_dbscan", cloud_xyz, n, nullptr, n, &f));
    // one cell grid: a cell about a radius long, by the rule of mi_remove_outliers' radius method
    const float ppc = c->tune.knn_points_per_cell > 0.f ? c->tune.knn_points_per_cell
                                                        : radius_points_per_cell(f.bbox, n, p->radius, c->tune.outlier_radius_cell);
    MI_TRY(search_front_index_and_order(c, b.front, clock, "mi_cluster_dbscan", ppc, &f));

    // host-side shape checks before the hand-written kernels run: every array they index is as long as the launches assume
    if (!search_front_fits(b.front, f) || !bufs.fits()) {
        set_error("internal: mi_cluster_dbscan buffers shorter than the launch");
        return MI_ERR_STATE;
    }
    const int fma = p->dist_mode == MI_DIST_FMA;
    const int need = min_points - 1;                                               // core: at least this many neighbours
    if (counted) {
        RadiusCountArgs ra{};
        ra.q = search_front_queries(b.front, f);
        ra.r2 = r2; ra.min_neighbours = need;
        ra.count = b.count.p;
        MI_HIP(radius_count(f.g, ra, fma, 1, c->stream));                          // early: the count stops at `need`
    }
    MI_HIP(cluster_identity(b.parent.p, n, c->stream));
    MI_TRY(clock.mark(8));

    MI_TRY(search_front_timed_launch(c, b.front, clock, [&] {
        ClusterLinkArgs a{};
        a.q = search_front_queries(b.front, f);
        a.r2 = r2; a.count = counted ? b.count.p : nullptr; a.need = need;
        a.parent = b.parent.p;
        return cluster_link(f.g, a, fma, c->stream);
    }));

    ClusterResolveArgs ra{};
    ra.q = search_front_queries(b.front, f);
    ra.r2 = r2; ra.count = counted ? b.count.p : nullptr; ra.need = need;
    ra.parent = b.parent.p; ra.root_of = b.root_of.p; ra.is_core = b.core.p;
    MI_HIP(cluster_resolve(f.g, ra, fma, c->stream));
    MI_TRY(clock.mark(6));

    MI_HIP(hipMemsetAsync(b.ostate.p, 0, 2 * sizeof(OutlierState), c->stream));
    MI_HIP(hipMemsetAsync(b.size.p, 0, sizeof(int) * np, c->stream));
    ClusterNumberArgs na{};
    na.n = n; na.root_of = b.root_of.p; na.size = b.size.p; na.min_size = min_size; na.max_size = max_size; na.keep = b.keep.p;
    na.roots = b.roots.p; na.state = b.ostate.p; na.rank = b.rank.p; na.sizes_out = cluster_sizes ? b.sizes_out.p : nullptr; na.cap = sizes_cap;
    na.labels = b.labels.p; na.labelled = n_grouped ? b.labelled.p : nullptr;
    MI_HIP(cluster_count_sizes(na, c->stream));
    OutlierCompactArgs ca{};
    ca.keep = b.keep.p; ca.n = n; ca.tile_counts = b.tile_counts.p; ca.out_index = b.roots.p; ca.state = b.ostate.p;
    MI_HIP(outlier_compact(ca, c->stream));                                        // the surviving roots, ascending; kept: their number
    MI_HIP(cluster_ranks(na, c->stream));
    MI_HIP(cluster_labels(na, c->stream));
    if (n_grouped) {                                                               // the labelled points, ascending; kept: their number
        OutlierCompactArgs ga{};
        ga.keep = b.labelled.p; ga.n = n; ga.tile_counts = b.tile_counts.p; ga.out_index = grouped_index ? b.group_a.p : nullptr; ga.state = b.ostate.p + 1;
        MI_HIP(outlier_compact(ga, c->stream));
    }

    // both counts once; nothing of the caller's has been written yet
    MI_TRY(compact_read_state(c, b.ostate.p, 2));
    MI_HIP(hipStreamSynchronize(c->stream));
    long long found, grouped = 0;
    const bool found_ok = compact_kept(c, 0, n, &found), grouped_ok = !n_grouped || compact_kept(c, 1, n, &grouped);
    if (!found_ok || !grouped_ok || (n_grouped && (found == 0) != (grouped == 0))) {
        set_error("internal: mi_cluster_dbscan counted %lld clusters and %lld labelled points among %d points", found, grouped, n);
        return MI_ERR_STATE;
    }
    const int* sorted = b.group_a.p;
    if (grouped_index && grouped > 0) {
        // stable by label over ascending indices: (label, index) order.  Ten bits per pass; labels of 2^30 and above take one more sort
        const int ng = (int)grouped;
        int bits = 10;
        while (bits < 30 && ((long long)1 << bits) < found) bits += 10;
        MI_HIP(cluster_group_keys(b.labels.p, b.group_a.p, ng, 0, b.keys_a.p, c->stream));
        MI_HIP(radix_sort_pairs_u32(b.sort_temp.p, b.keys_a.p, b.keys_b.p, b.group_a.p, b.group_b.p, ng, bits, c->stream));
        sorted = b.group_b.p;
        if (found > ((long long)1 << 30)) {
            MI_HIP(cluster_group_keys(b.labels.p, b.group_b.p, ng, 30, b.keys_a.p, c->stream));
            MI_HIP(radix_sort_pairs_u32(b.sort_temp.p, b.keys_a.p, b.keys_b.p, b.group_b.p, b.group_a.p, ng, 10, c->stream));
            sorted = b.group_a.p;
        }
    }
    MI_TRY(bufs.download(c->stream));
    const size_t nsizes = (size_t)std::min<long long>(found, sizes_cap);
    if (cluster_sizes && nsizes > 0) MI_HIP(hipMemcpyAsync(cluster_sizes, b.sizes_out.p, sizeof(int) * nsizes, hipMemcpyDeviceToHost, c->stream));
    if (grouped_index && grouped > 0) MI_HIP(hipMemcpyAsync(grouped_index, sorted, sizeof(int) * (size_t)grouped, hipMemcpyDeviceToHost, c->stream));
    MI_HIP(hipStreamSynchronize(c->stream));
    *n_clusters = (int)found;
    if (n_grouped) *n_grouped = (int)grouped;
    MI_TRY(clock.mark(9));
    clock.finish();
    b.ms[0] = t[0]; b.ms[1] = t[1] + t[2]; b.ms[2] = t[3] + t[4]; b.ms[3] = t[8]; b.ms[4] = t[5]; b.ms[5] = t[6]; b.ms[6] = t[9]; b.ms[7] = t[7];
    return MI_OK;
}

extern "C" int mi_cluster_dbscan_times(mi_ctx* c, double out_ms[MI_CLUSTER_STAGES]) { return stage_times("mi_cluster_dbscan_times", c ? c->cluster.ms : nullptr, out_ms); }
