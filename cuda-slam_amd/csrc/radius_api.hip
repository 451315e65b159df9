// mi_radius_search behind the C ABI: argument checks, the reserves of the call's own buffers in the context, the search front end
// (search_front.hip: uploads, input check and its one read-back, ONE cell grid over the cloud with cells about one radius long, the curve
// order of the queries -- the cloud's own in self mode, their own where they are a cloud of their own), the count (K15's launch in self mode,
// its twin for a separate query set), K51's scan and the one read-back of the total, and -- where lists were asked for and fit the caller's
// capacity -- their reserves, K52's fill, K53's sort, K54's unpack and the download.  The lists' buffers are the only ones reserved behind the
// uploads: their length is what the call computes.
#include <hip/hip_runtime.h>

#include <cmath>

#include "context.h"

using namespace mislam;

extern "C" int mi_radius_search(mi_ctx* c, const float* query_xyz, int n, const float* cloud_xyz, int m, float radius, int dist_mode, int sorted,
                                long long* offsets, int* idx, float* d2, long long capacity, long long* total)
{
    if (!c) { set_error("mi_radius_search: null context"); return MI_ERR_INVALID_ARG; }
    if (!cloud_xyz || !offsets || !total) { set_error("mi_radius_search: null cloud_xyz, offsets or total"); return MI_ERR_INVALID_ARG; }
    if (n < 1 || m < 1) { set_error("mi_radius_search: empty query set or cloud (n = %d, m = %d)", n, m); return MI_ERR_INVALID_ARG; }
    const bool self = query_xyz == nullptr;
    if (self && n != m) { set_error("mi_radius_search: self mode (query_xyz == NULL) needs n == m (n = %d, m = %d)", n, m); return MI_ERR_INVALID_ARG; }
    if (dist_mode != MI_DIST_CPU_ROUNDING && dist_mode != MI_DIST_FMA) { set_error("mi_radius_search: bad dist_mode %d", dist_mode); return MI_ERR_INVALID_ARG; }
    if (sorted != 0 && sorted != 1) { set_error("mi_radius_search: sorted = %d outside {0, 1}", sorted); return MI_ERR_INVALID_ARG; }
    const float r2 = radius * radius;                                                  // one IEEE fp32 multiplication (-ffp-contract=off)
    if (!(std::isfinite(radius) && radius > 0.f)) { set_error("mi_radius_search: radius %g is NaN, infinite or not positive", (double)radius); return MI_ERR_INVALID_ARG; }
    if (!std::isfinite(r2)) { set_error("mi_radius_search: the square of radius %g is not finite", (double)radius); return MI_ERR_INVALID_ARG; }
    if (d2 && !idx) { set_error("mi_radius_search: d2 given without idx"); return MI_ERR_INVALID_ARG; }
    if (!idx && capacity != 0) { set_error("mi_radius_search: capacity = %lld without idx (a counts-only call takes capacity 0)", capacity); return MI_ERR_INVALID_ARG; }
    if (idx && (capacity < 1 || capacity > MI_RADIUS_MAX_TOTAL)) {
        set_error("mi_radius_search: capacity = %lld outside [1, MI_RADIUS_MAX_TOTAL = %lld] with idx given", capacity, (long long)MI_RADIUS_MAX_TOTAL);
        return MI_ERR_INVALID_ARG;
    }
    if (c->distributed()) { set_error("mi_radius_search: single-GPU contexts only"); return MI_ERR_STATE; }
    MI_ENTER(c);
    mi_ctx::RadiusBuffers& b = c->radius;
    // the front end books its stages as every search call's (context.h); t[8] is the scan and its read-back; the count, the fill and the sort
    // each pass through slot 5: regrouped into the eight slots of mi_radius_search_times at the end
    double t[9] = {0};
    StageClock clock(c, t);

    const size_t rows = (size_t)n;
    CallBuffers bufs;                  // (in the order of the download; the lists join once their length is known)
    MI_TRY(search_front_reserve(b.front, rows, (size_t)m, self));
    MI_TRY(bufs.need(b.count, rows)); MI_TRY(bufs.need(b.tile_sums, (size_t)radius_scan_tiles(n))); MI_TRY(bufs.need(b.offsets, rows + 1, offsets));
    if (idx) MI_TRY(bufs.need(b.mismatch, 1));
    MI_TRY(clock.mark(0));

    SearchFront f;
    MI_TRY(search_front_upload_and_check(c, b.front, clock, "mi_radius_search", cloud_xyz, m, query_xyz, n, &f));
    // a cell about one radius long, by the rule of mi_remove_outliers' radius method
    const float ppc = c->tune.knn_points_per_cell > 0.f ? c->tune.knn_points_per_cell : radius_points_per_cell(f.bbox, m, radius, c->tune.outlier_radius_cell);
    MI_TRY(search_front_index_and_order(c, b.front, clock, "mi_radius_search", ppc, &f));

    // host-side shape checks before the hand-written kernels run: every array they index is as long as the launches assume
    if (!search_front_fits(b.front, f) || !bufs.fits()) {
        set_error("internal: mi_radius_search buffers shorter than the launch");
        return MI_ERR_STATE;
    }
    b.grid_dims[0] = f.g.nx; b.grid_dims[1] = f.g.ny; b.grid_dims[2] = f.g.nz;
    const int fma = dist_mode == MI_DIST_FMA;
    const SearchQueries q = search_front_queries(b.front, f);
    MI_TRY(search_front_timed_launch(c, b.front, clock, [&] {
        if (!self) return radius_query_count(f.g, q, r2, b.count.p, fma, c->stream);
        RadiusCountArgs a{};
        a.q = q;
        a.r2 = r2; a.min_neighbours = 1;
        a.count = b.count.p;
        return radius_count(f.g, a, fma, 0, c->stream);
    }));
    // search_front_timed_launch books slot 5 (with profiling on: the launch's own HIP-event time); the fill and the sort go through it too
    const double count_ms = t[5];
    double fill_ms = 0.0, sort_ms = 0.0;
    t[5] = 0.0;

    // the offsets in the caller's row order, and the one round trip in front of the lists: the total
    MI_HIP(radius_scan_offsets(b.count.p, n, b.tile_sums.p, b.offsets.p, c->stream));
    long long* h_total = reinterpret_cast<long long*>(c->h_scratch);
    MI_HIP(hipMemcpyAsync(h_total, b.offsets.p + rows, sizeof(long long), hipMemcpyDeviceToHost, c->stream));
    MI_HIP(hipStreamSynchronize(c->stream));
    const long long found = *h_total;
    if (found < 0 || found > (long long)n * (long long)m) { set_error("internal: mi_radius_search counted %lld members for %d queries over %d points", found, n, m); return MI_ERR_STATE; }
    MI_TRY(clock.mark(8));

    const bool lists = idx && found <= capacity;                                     // (found <= capacity <= MI_RADIUS_MAX_TOTAL)
    const size_t entries = (size_t)found;
    if (lists && found > 0) {
        MI_TRY(bufs.need(b.keys, entries)); MI_TRY(bufs.need(b.out_idx, entries, idx)); MI_TRY(bufs.result(b.out_d2, entries, d2));
        MI_TRY(clock.mark(0));
        if (!bufs.fits()) {
            set_error("internal: mi_radius_search lists shorter than the launch");
            return MI_ERR_STATE;
        }
        // an unsorted row is what the walk met: every cell's points by index first, so that it meets the same on every call (the count,
        // a sum over the cells, did not care; only a call that writes lists pays for this)
        if (!sorted) {
            MI_HIP(radius_order_cells(b.front.cells.start.p, (long long)f.n_cells, b.front.cells.pts.p, c->stream));
            MI_TRY(clock.mark(4));
        }
        MI_HIP(hipMemsetAsync(b.mismatch.p, 0, sizeof(int), c->stream));
        MI_TRY(search_front_timed_launch(c, b.front, clock, [&] {
            RadiusFillArgs a{};
            a.q = q; a.self = self ? 1 : 0;
            a.r2 = r2;
            a.offsets = b.offsets.p; a.keys = b.keys.p; a.mismatch = b.mismatch.p;
            return radius_fill(f.g, a, fma, c->stream);
        }));
        fill_ms = t[5]; t[5] = 0.0;
        if (sorted) {
            MI_TRY(search_front_timed_launch(c, b.front, clock, [&] { return radius_sort_rows(b.offsets.p, (long long)n, b.keys.p, c->stream); }));
            sort_ms = t[5]; t[5] = 0.0;
        }
        MI_HIP(radius_unpack(b.keys.p, found, b.out_idx.p, d2 ? b.out_d2.p : nullptr, c->stream));
        // both walks are the same code over the same grid; should they ever disagree, the caller hears of it before any list is written
        int* h_mismatch = reinterpret_cast<int*>(c->h_scratch);
        MI_HIP(hipMemcpyAsync(h_mismatch, b.mismatch.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        MI_HIP(hipStreamSynchronize(c->stream));
        if (*h_mismatch != 0) { set_error("internal: mi_radius_search's fill walk met another number of members than its count"); return MI_ERR_STATE; }
    }

    MI_TRY(bufs.download(c->stream));
    MI_HIP(hipStreamSynchronize(c->stream));
    *total = found;
    MI_TRY(clock.mark(6));
    clock.finish();
    b.ms[0] = t[0]; b.ms[1] = t[1] + t[2] + t[3] + t[4]; b.ms[2] = count_ms; b.ms[3] = t[8]; b.ms[4] = fill_ms; b.ms[5] = sort_ms; b.ms[6] = t[6]; b.ms[7] = t[7];
    return MI_OK;
}

extern "C" int mi_radius_search_times(mi_ctx* c, double out_ms[MI_RADIUS_STAGES]) { return stage_times("mi_radius_search_times", c ? c->radius.ms : nullptr, out_ms); }

extern "C" int mi_selftest_radius_grid(mi_ctx* c, int dims[3])
{
    if (!c || !dims) { set_error("mi_selftest_radius_grid: null argument"); return MI_ERR_INVALID_ARG; }
    for (int i = 0; i < 3; i++) dims[i] = c->radius.grid_dims[i];
    return MI_OK;
}
