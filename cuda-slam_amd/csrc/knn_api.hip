// mi_knn_search behind the C ABI: argument checks, the reserves of the call's own buffers in the context, the search front end
// (search_front.hip: uploads, input check and its one read-back, the cell grid over the cloud, the curve order of the queries), the
// arguments and the launch of knn_kernels.hip's search, and the download.
#include <hip/hip_runtime.h>

#include "context.h"

using namespace mislam;

static_assert(KNN_MAX_K == MI_KNN_MAX_K, "the kernels' list sizes cover MI_KNN_MAX_K");

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

    const size_t np = (size_t)n, rows = np * (size_t)k;
    CallBuffers bufs;
    MI_TRY(search_front_reserve(b.front, np, (size_t)m, self));
    MI_TRY(bufs.result(b.out_idx, rows, idx)); MI_TRY(bufs.result(b.out_d2, rows, d2)); MI_TRY(bufs.result(b.out_count, np, count));
    MI_TRY(clock.mark(0));

    SearchFront f;
    MI_TRY(search_front_upload_and_check(c, b.front, clock, "mi_knn_search", cloud_xyz, m, query_xyz, n, &f));
    const float ppc = c->tune.knn_points_per_cell > 0.f ? c->tune.knn_points_per_cell : knn_default_points_per_cell(k);
    MI_TRY(search_front_index_and_order(c, b.front, clock, "mi_knn_search", ppc, &f));

    KnnSearchArgs a{};
    const SearchQueries q = search_front_queries(b.front, f);
    a.qx = q.x; a.qy = q.y; a.qz = q.z; a.order = q.order;      // (the kernel keeps the fields of its own: kernels.h)
    a.n = q.n; a.k = k; a.self = self ? 1 : 0; a.max_d2 = max_distance_squared;
    for (int i = 0; i < 3; i++) a.hi[i] = q.hi[i];
    a.idx = b.out_idx.p; a.d2 = d2 ? b.out_d2.p : nullptr; a.count = count ? b.out_count.p : nullptr;
    // host-side shape checks before the hand-written kernel runs: every array it indexes is as long as the launch assumes
    if (!search_front_fits(b.front, f) || !bufs.fits()) {
        set_error("internal: mi_knn_search buffers shorter than the launch");
        return MI_ERR_STATE;
    }
    MI_TRY(search_front_timed_launch(c, b.front, clock, [&] { return knn_search(f.g, a, dist_mode == MI_DIST_FMA, c->stream); }));

    MI_TRY(bufs.download(c->stream));
    MI_HIP(hipStreamSynchronize(c->stream));
    MI_TRY(clock.mark(6));
    clock.finish();
    return MI_OK;
}

extern "C" int mi_knn_search_times(mi_ctx* c, double out_ms[MI_KNN_STAGES]) { return stage_times("mi_knn_search_times", c ? c->knn.ms : nullptr, out_ms); }
