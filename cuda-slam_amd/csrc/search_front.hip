// The front end of a search over a cloud's cell grid, stated once for mi_knn_search, mi_estimate_normals and mi_remove_outliers (declared in
// context.h): the common reserves, the uploads, the input check and its one read-back (knn_check_inputs), the cell grid over the cloud
// (grid_reserve / grid_build_into of nn_grid.h with the call's buffers), the curve order of the queries (morton_order / permute_soa of
// nn_tree.h), the views of the queries and the cloud that a search kernel is handed (search_front_queries, search_front_cloud), and for the
// calls that bring normals along their upload and check (search_front_enqueue_normals, search_front_refuse_normals).  A driver keeps its own
// argument checks, its own reserves, the rest of its kernel's arguments, its launch (search_front_timed_launch) and its download.  `who` is the entry point's name: every message a call can refuse with reads the same in all three but for it.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "context.h"

namespace mislam {

static_assert(sizeof(KnnState) <= 64 * sizeof(float), "KnnState must fit the context's pinned scratch");

// Points per cell of the grid for a search of k neighbours, unless MISLAM_KNN_POINTS_PER_CELL says otherwise.
// A lane stops behind shell r once r cells are longer than its k-th distance, so the cell size trades candidates tested (27 cells of k / 2 points) against
// shells walked.  An estimate: the sweep of tools/knn_bench.py --sweep has not been run yet.
float knn_default_points_per_cell(int k) { return std::max(1.0f, 0.5f * (float)k); }

// Points per cell of a fixed-radius search's grid (mi_remove_outliers' radius method; mi_iss_keypoints, with the larger of its two
// radii): the number that makes a cell's edge `cell_in_radii` radii long (1 unless MISLAM_OUTLIER_RADIUS_CELL says otherwise), so that
// a ball reaches into the 27 cells around its point's and rarely further.  An axis
// shorter than that edge is one layer of cells.  Bounded below by the k-NN rule's floor (at most one cell per point: a small radius in a
// sparse cloud must not buy more cells than points) and above by n (one cell); grid_plan keeps the counts within GRID_MAX_DIM.
// A rule by reasoning, not by measurement.
float radius_points_per_cell(const float bbox[6], int n, float radius, float cell_in_radii)
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

int search_front_reserve(SearchFrontBuffers& b, size_t n, size_t m, bool self)
{
    MI_TRY(b.staging.reserve(3 * std::max(n, m)));
    MI_TRY(b.cx.reserve(m)); MI_TRY(b.cy.reserve(m)); MI_TRY(b.cz.reserve(m));
    if (!self) { MI_TRY(b.ux.reserve(n)); MI_TRY(b.uy.reserve(n)); MI_TRY(b.uz.reserve(n)); }
    MI_TRY(b.qx.reserve(n)); MI_TRY(b.qy.reserve(n)); MI_TRY(b.qz.reserve(n));
    MI_TRY(b.range_lo_hi.reserve(2 * 6 * KNN_RANGE_BLOCKS)); MI_TRY(b.range_bad.reserve(2 * KNN_RANGE_BLOCKS)); MI_TRY(b.state.reserve(1));
    MI_TRY(b.order.reserve(n));
    return MI_OK;
}

int search_front_upload_and_check(mi_ctx* c, SearchFrontBuffers& b, StageClock& clock, const char* who, const float* cloud_xyz, int m,
                                  const float* query_xyz, int n, SearchFront* f, const char* cloud_name, const char* query_name)
{
    const bool self = query_xyz == nullptr;
    MI_TRY(host_to_device(c, b.staging.p, cloud_xyz, sizeof(float) * 3 * (size_t)m));
    MI_HIP(aos_to_soa(b.staging.p, m, m, b.cx.p, b.cy.p, b.cz.p, nullptr, c->stream));
    if (!self) {
        MI_TRY(host_to_device(c, b.staging.p, query_xyz, sizeof(float) * 3 * (size_t)n));
        MI_HIP(aos_to_soa(b.staging.p, n, n, b.ux.p, b.uy.p, b.uz.p, nullptr, c->stream));
    }
    f->n = n; f->m = m;
    f->ux = self ? b.cx.p : b.ux.p; f->uy = self ? b.cy.p : b.uy.p; f->uz = self ? b.cz.p : b.uz.p;
    MI_TRY(clock.mark(1));

    MI_HIP(knn_check_inputs(b.cx.p, b.cy.p, b.cz.p, m, self ? nullptr : f->ux, f->uy, f->uz, n, b.range_lo_hi.p, b.range_bad.p, b.state.p, c->stream));
    KnnState* st = reinterpret_cast<KnnState*>(c->h_scratch);     // (pinned, 256 bytes)
    MI_HIP(hipMemcpyAsync(st, b.state.p, sizeof(KnnState), hipMemcpyDeviceToHost, c->stream));
    MI_HIP(hipStreamSynchronize(c->stream));
    MI_TRY(clock.mark(2));
    // everything that can refuse the input is known here, before any output array has been touched
    if (st->bad_cloud != KNN_NO_POINT) {
        set_error("%s: %s point %d has a non-finite coordinate or one above 1e18 in magnitude", who, cloud_name, st->bad_cloud);
        return MI_ERR_INVALID_ARG;
    }
    if (st->bad_query != KNN_NO_POINT) {
        set_error("%s: %s point %d has a non-finite coordinate or one above 1e18 in magnitude", who, query_name, st->bad_query);
        return MI_ERR_INVALID_ARG;
    }
    for (int i = 0; i < 3; i++) { f->bbox[i] = st->lo[i]; f->bbox[3 + i] = st->hi[i]; }
    return MI_OK;
}

int search_front_index_and_order(mi_ctx* c, SearchFrontBuffers& b, StageClock& clock, const char* who, float points_per_cell, SearchFront* f)
{
    // the cell grid over the cloud
    NnGridView& g = f->g;
    MI_TRY(grid_reserve(b.cells, f->bbox, f->m, 0, points_per_cell, &g));
    MI_TRY(clock.mark(0));
    // (grid_plan clamps the counts to [1, GRID_MAX_DIM], so the reserves above were sane whatever the box; a cell size that left fp32 can still show here)
    if (g.nx < 1 || g.ny < 1 || g.nz < 1 || g.nx > GRID_MAX_DIM || g.ny > GRID_MAX_DIM || g.nz > GRID_MAX_DIM || !(g.inv_h > 0.f) || !(g.h_lo > 0.f)) {
        set_error("internal: %s planned a %d x %d x %d grid", who, g.nx, g.ny, g.nz);
        return MI_ERR_STATE;
    }
    f->n_cells = (size_t)g.nx * g.ny * g.nz;
    MI_TRY(grid_build_into(b.cells, g, b.cx.p, b.cy.p, b.cz.p, f->m, c->stream));
    MI_TRY(clock.mark(3));
    return search_front_order(c, b, clock, f);
}

int search_front_order(mi_ctx* c, SearchFrontBuffers& b, StageClock& clock, SearchFront* f)
{
    // the queries along their curve: order[s] = the caller's index of sorted slot s
    MortonArgs ma{};
    MI_TRY(morton_args(b.morton, f->ux, f->uy, f->uz, f->n, b.order.p, &ma));
    MI_HIP(morton_order(ma, c->stream));
    MI_HIP(permute_soa(f->ux, f->uy, f->uz, b.order.p, f->n, f->n, b.qx.p, b.qy.p, b.qz.p, c->stream));
    MI_TRY(clock.mark(4));
    return MI_OK;
}

int search_front_enqueue_normals(mi_ctx* c, SearchFrontBuffers& b, const float* normals_xyz, int m, float* nx, float* ny, float* nz, float4* packed,
                                 KnnState* nstate)
{
    MI_TRY(host_to_device(c, b.staging.p, normals_xyz, sizeof(float) * 3 * (size_t)m));
    MI_HIP(aos_to_soa(b.staging.p, m, m, nx, ny, nz, packed, c->stream));
    MI_HIP(knn_check_inputs(nx, ny, nz, m, nullptr, nullptr, nullptr, 0, b.range_lo_hi.p, b.range_bad.p, nstate, c->stream));
    return MI_OK;
}

int search_front_refuse_normals(mi_ctx* c, StageClock& clock, const char* who, const char* name, const KnnState* nstate)
{
    KnnState ns;
    MI_HIP(hipMemcpyAsync(&ns, nstate, sizeof ns, hipMemcpyDeviceToHost, c->stream));
    MI_HIP(hipStreamSynchronize(c->stream));
    MI_TRY(clock.mark(2));
    if (ns.bad_cloud != KNN_NO_POINT) {
        set_error("%s: %s normal %d has a non-finite component or one above 1e18 in magnitude", who, name, ns.bad_cloud);
        return MI_ERR_INVALID_ARG;
    }
    return MI_OK;
}

SearchQueries search_front_queries(const SearchFrontBuffers& b, const SearchFront& f)
{
    SearchQueries q{};
    q.x = b.qx.p; q.y = b.qy.p; q.z = b.qz.p; q.order = b.order.p;
    q.n = f.n;
    for (int i = 0; i < 3; i++) q.hi[i] = f.bbox[3 + i];
    return q;
}

SearchCloud search_front_cloud(const SearchFrontBuffers& b) { return SearchCloud{b.cx.p, b.cy.p, b.cz.p}; }

bool search_front_fits(const SearchFrontBuffers& b, const SearchFront& f)
{
    const size_t n = (size_t)f.n, m = (size_t)f.m;
    return b.qx.cap >= n && b.qy.cap >= n && b.qz.cap >= n && b.order.cap >= n && b.cx.cap >= m && b.cy.cap >= m && b.cz.cap >= m &&
           b.cells.start.cap >= f.n_cells + 1 && b.cells.pts.cap >= m;
}

void search_front_destroy_events(mi_ctx* c)
{
    for (SearchFrontBuffers* b : {&c->knn.front, &c->normals.front, &c->outlier.front, &c->plane.front, &c->cov.front, &c->gicp.front, &c->fpfh.front, &c->iss.front, &c->cluster.front, &c->segment.front, &c->colorgrad.front, &c->color.front, &c->mls.front, &c->radius.front, &c->eval.front})
        for (hipEvent_t e : b->ev) if (e) (void)hipEventDestroy(e);
}

}  // namespace mislam
