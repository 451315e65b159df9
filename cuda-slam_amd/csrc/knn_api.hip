// mi_knn_search behind the C ABI: argument checks, the call's own buffers in the context, the uploads, the input check and its one
// read-back, the cell grid over the cloud (grid_plan / grid_build of nn_grid.h with the call's buffers), the curve order of the
// queries (morton_order / permute_soa of nn_tree.h), the launch of knn_kernels.hip's search and the download.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "context.h"

using namespace mislam;

static_assert(KNN_MAX_K == MI_KNN_MAX_K, "the kernels' list sizes cover MI_KNN_MAX_K");

// Points per cell of the grid for a search of k neighbours, unless MISLAM_KNN_POINTS_PER_CELL says otherwise (mi_estimate_normals uses the same rule).
// A lane stops behind shell r once r cells are longer than its k-th distance, so the cell size trades candidates tested (27 cells of k / 2 points) against
// shells walked.  An estimate: the sweep of tools/knn_bench.py --sweep has not been run yet.
float mislam::knn_default_points_per_cell(int k) { return std::max(1.0f, 0.5f * (float)k); }

extern "C" int mi_knn_search(mi_ctx* c, const float* query_xyz, int n, const float* cloud_xyz, int m, int k, int dist_mode,
                             float max_distance_squared, int* idx, float* d2, int* count)
{
    if (!c) { set_error("mi_knn_search: null context"); return MI_ERR_INVALID_ARG; }
    if (!cloud_xyz || !idx) { set_error("mi_knn_search: null cloud_xyz or idx"); return MI_ERR_INVALID_ARG; }
    if (n < 1 || m < 1) { set_error("mi_knn_search: empty query set or cloud (n = %d, m = %d)", n, m); return MI_ERR_INVALID_ARG; }
    if (k < 1 || k > MI_KNN_MAX_K) { set_error("mi_knn_search: k = %d outside [1, %d]", k, MI_KNN_MAX_K); return MI_ERR_INVALID_ARG; }
    if (dist_mode != MI_DIST_CPU_ROUNDING && dist_mode != MI_DIST_FMA) { set_error("mi_knn_search: bad dist_mode %d", dist_mode); return MI_ERR_INVALID_ARG; }
    if (!(max_distance_squared >= 0.f)) { set_error("mi_knn_search: max_distance_squared %g is NaN or negative", (double)max_distance_squared); return MI_ERR_INVALID_ARG; }
    const bool self = query_xyz == nullptr;
    if (self && n != m) { set_error("mi_knn_search: self mode (query_xyz == NULL) needs n == m (n = %d, m = %d)", n, m); return MI_ERR_INVALID_ARG; }
    if (c->distributed()) { set_error("mi_knn_search: single-GPU contexts only"); return MI_ERR_STATE; }
    MI_ENTER(c);
    mi_ctx::KnnBuffers& b = c->knn;
    StageClock clock(c, b.ms);         // mi_knn_search_times

    const size_t np = (size_t)n, mp = (size_t)m, rows = np * (size_t)k;
    MI_TRY(b.staging.reserve(3 * std::max(np, mp)));
    MI_TRY(b.cx.reserve(mp)); MI_TRY(b.cy.reserve(mp)); MI_TRY(b.cz.reserve(mp));
    if (!self) { MI_TRY(b.ux.reserve(np)); MI_TRY(b.uy.reserve(np)); MI_TRY(b.uz.reserve(np)); }
    MI_TRY(b.qx.reserve(np)); MI_TRY(b.qy.reserve(np)); MI_TRY(b.qz.reserve(np));
    MI_TRY(b.range_lo_hi.reserve(2 * 6 * KNN_RANGE_BLOCKS)); MI_TRY(b.range_bad.reserve(2 * KNN_RANGE_BLOCKS)); MI_TRY(b.state.reserve(1));
    MI_TRY(b.order.reserve(np));
    MI_TRY(b.out_idx.reserve(rows));
    if (d2) MI_TRY(b.out_d2.reserve(rows));
    if (count) MI_TRY(b.out_count.reserve(np));
    MI_TRY(clock.mark(0));

    MI_TRY(host_to_device(c, b.staging.p, cloud_xyz, sizeof(float) * 3 * mp));
    MI_HIP(aos_to_soa(b.staging.p, m, m, b.cx.p, b.cy.p, b.cz.p, nullptr, c->stream));
    if (!self) {
        MI_TRY(host_to_device(c, b.staging.p, query_xyz, sizeof(float) * 3 * np));
        MI_HIP(aos_to_soa(b.staging.p, n, n, b.ux.p, b.uy.p, b.uz.p, nullptr, c->stream));
    }
    const float *ux = self ? b.cx.p : b.ux.p, *uy = self ? b.cy.p : b.uy.p, *uz = self ? b.cz.p : b.uz.p;
    MI_TRY(clock.mark(1));

    MI_HIP(knn_check_inputs(b.cx.p, b.cy.p, b.cz.p, m, self ? nullptr : ux, uy, uz, n, b.range_lo_hi.p, b.range_bad.p, b.state.p, c->stream));
    KnnState* st = reinterpret_cast<KnnState*>(c->h_scratch);     // (pinned, 256 bytes)
    static_assert(sizeof(KnnState) <= 64 * sizeof(float), "KnnState must fit the context's pinned scratch");
    MI_HIP(hipMemcpyAsync(st, b.state.p, sizeof(KnnState), hipMemcpyDeviceToHost, c->stream));
    MI_HIP(hipStreamSynchronize(c->stream));
    MI_TRY(clock.mark(2));
    // everything that can refuse the input is known here, before any output array has been touched
    if (st->bad_cloud != KNN_NO_POINT) {
        set_error("mi_knn_search: cloud_xyz point %d has a non-finite coordinate or one above 1e18 in magnitude", st->bad_cloud);
        return MI_ERR_INVALID_ARG;
    }
    if (st->bad_query != KNN_NO_POINT) {
        set_error("mi_knn_search: query_xyz point %d has a non-finite coordinate or one above 1e18 in magnitude", st->bad_query);
        return MI_ERR_INVALID_ARG;
    }

    // the cell grid over the cloud
    const float bbox[6] = {st->lo[0], st->lo[1], st->lo[2], st->hi[0], st->hi[1], st->hi[2]};
    const float ppc = c->tune.knn_points_per_cell > 0.f ? c->tune.knn_points_per_cell : knn_default_points_per_cell(k);
    NnGridView g{};
    MI_TRY(grid_reserve(b.cells, bbox, m, 0, ppc, &g));
    MI_TRY(clock.mark(0));
    // (grid_plan clamps the counts to [1, GRID_MAX_DIM], so the reserves above were sane whatever the box; a cell size that left fp32 can still show here)
    if (g.nx < 1 || g.ny < 1 || g.nz < 1 || g.nx > GRID_MAX_DIM || g.ny > GRID_MAX_DIM || g.nz > GRID_MAX_DIM || !(g.inv_h > 0.f) || !(g.h_lo > 0.f)) {
        set_error("internal: mi_knn_search planned a %d x %d x %d grid", g.nx, g.ny, g.nz);
        return MI_ERR_STATE;
    }
    const size_t n_cells = (size_t)g.nx * g.ny * g.nz;
    MI_TRY(grid_build_into(b.cells, g, b.cx.p, b.cy.p, b.cz.p, m, c->stream));
    MI_TRY(clock.mark(3));

    // the queries along their curve: order[s] = the caller's index of sorted slot s
    MortonArgs ma{};
    MI_TRY(morton_args(b.morton, ux, uy, uz, n, b.order.p, &ma));
    MI_HIP(morton_order(ma, c->stream));
    MI_HIP(permute_soa(ux, uy, uz, b.order.p, n, n, b.qx.p, b.qy.p, b.qz.p, c->stream));
    MI_TRY(clock.mark(4));

    KnnSearchArgs a{};
    a.qx = b.qx.p; a.qy = b.qy.p; a.qz = b.qz.p; a.order = b.order.p;
    a.n = n; a.k = k; a.self = self ? 1 : 0; a.max_d2 = max_distance_squared;
    for (int i = 0; i < 3; i++) a.hi[i] = bbox[3 + i];
    a.idx = b.out_idx.p; a.d2 = d2 ? b.out_d2.p : nullptr; a.count = count ? b.out_count.p : nullptr;
    // host-side shape checks before the hand-written kernel runs: every array it indexes is as long as the launch assumes
    if (b.qx.cap < np || b.order.cap < np || b.out_idx.cap < rows || (d2 && b.out_d2.cap < rows) || (count && b.out_count.cap < np) ||
        b.cells.start.cap < n_cells + 1 || b.cells.pts.cap < mp) {
        set_error("internal: mi_knn_search buffers shorter than the launch");
        return MI_ERR_STATE;
    }
    const bool timed = c->prof.on;
    if (timed) {
        for (hipEvent_t& e : b.ev)
            if (!e) MI_HIP(hipEventCreate(&e));
        MI_HIP(hipEventRecord(b.ev[0], c->stream));
    }
    MI_HIP(knn_search(g, a, dist_mode == MI_DIST_FMA, c->stream));
    if (timed) MI_HIP(hipEventRecord(b.ev[1], c->stream));
    MI_TRY(clock.mark(5));
    if (timed) {
        float ms = 0.f;
        MI_HIP(hipEventElapsedTime(&ms, b.ev[0], b.ev[1]));
        b.ms[5] = (double)ms;
    }

    MI_HIP(hipMemcpyAsync(idx, b.out_idx.p, sizeof(int) * rows, hipMemcpyDeviceToHost, c->stream));
    if (d2) MI_HIP(hipMemcpyAsync(d2, b.out_d2.p, sizeof(float) * rows, hipMemcpyDeviceToHost, c->stream));
    if (count) MI_HIP(hipMemcpyAsync(count, b.out_count.p, sizeof(int) * np, hipMemcpyDeviceToHost, c->stream));
    MI_HIP(hipStreamSynchronize(c->stream));
    MI_TRY(clock.mark(6));
    clock.finish();
    return MI_OK;
}

extern "C" int mi_knn_search_times(mi_ctx* c, double out_ms[MI_KNN_STAGES])
{
    if (!c || !out_ms) { set_error("mi_knn_search_times: null argument"); return MI_ERR_INVALID_ARG; }
    for (int i = 0; i < MI_KNN_STAGES; i++) out_ms[i] = c->knn.ms[i];
    return MI_OK;
}
