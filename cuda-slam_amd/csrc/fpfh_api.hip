// mi_fpfh_features behind the C ABI: argument checks, the reserves of the call's own buffers in the context, the normals' upload and input
// check, the search front end in self mode (search_front.hip: upload, input check and its one read-back, the cell grid over the cloud
// under mi_knn_search's points-per-cell rule, the curve order), the arguments and the two launches of fpfh_kernels.hip, and the download
// of what was asked for.
#include <hip/hip_runtime.h>

#include "context.h"
#include "fpfh_pair.hpp"

using namespace mislam;

static_assert(FPFH_BINS == MI_FPFH_BINS && FPFH_DIM == MI_FPFH_DIM, "fpfh_pair.hpp mirrors MI_FPFH_*");

extern "C" int mi_fpfh_features(mi_ctx* c, const float* cloud_xyz, const float* normals_xyz, int n, int k, int dist_mode, float max_distance_squared,
                                float* fpfh33, unsigned char* spfh_counts33, int* count)
{
    const char* who = "mi_fpfh_features";
    if (!c) { set_error("%s: null context", who); return MI_ERR_INVALID_ARG; }
    if (!cloud_xyz || !normals_xyz || !fpfh33) { set_error("%s: null cloud_xyz, normals_xyz or fpfh33", who); return MI_ERR_INVALID_ARG; }
    if (n < 1) { set_error("%s: empty cloud (n = %d)", who, n); return MI_ERR_INVALID_ARG; }
    if (k < 1 || k > MI_KNN_MAX_K) { set_error("%s: k = %d outside [1, %d]", who, k, MI_KNN_MAX_K); return MI_ERR_INVALID_ARG; }
    if (dist_mode != MI_DIST_CPU_ROUNDING && dist_mode != MI_DIST_FMA) { set_error("%s: bad dist_mode %d", who, dist_mode); return MI_ERR_INVALID_ARG; }
    if (!(max_distance_squared >= 0.f)) { set_error("%s: max_distance_squared %g is NaN or negative", who, (double)max_distance_squared); return MI_ERR_INVALID_ARG; }
    if (c->distributed()) { set_error("%s: single-GPU contexts only", who); return MI_ERR_STATE; }
    MI_ENTER(c);
    mi_ctx::FpfhBuffers& b = c->fpfh;
    StageClock clock(c, b.ms);         // mi_fpfh_features_times

    const size_t np = (size_t)n, rows = np * (size_t)k;
    CallBuffers bufs;
    MI_TRY(search_front_reserve(b.front, np, np, true));
    MI_TRY(bufs.need(b.nx, np)); MI_TRY(bufs.need(b.ny, np)); MI_TRY(bufs.need(b.nz, np)); MI_TRY(bufs.need(b.nstate, 1));
    MI_TRY(bufs.need(b.keys, rows)); MI_TRY(bufs.need(b.packed, FPFH_WORDS * np));
    MI_TRY(bufs.result(b.out_fpfh, FPFH_DIM * np, fpfh33)); MI_TRY(bufs.result(b.out_counts, FPFH_DIM * np, spfh_counts33)); MI_TRY(bufs.result(b.out_count, np, count));
    MI_TRY(clock.mark(0));

    MI_TRY(search_front_enqueue_normals(c, b.front, normals_xyz, n, b.nx.p, b.ny.p, b.nz.p, nullptr, b.nstate.p));
    SearchFront f;
    MI_TRY(search_front_upload_and_check(c, b.front, clock, who, cloud_xyz, n, nullptr, n, &f));
    MI_TRY(search_front_refuse_normals(c, clock, who, "normals_xyz", b.nstate.p));
    const float ppc = c->tune.knn_points_per_cell > 0.f ? c->tune.knn_points_per_cell : knn_default_points_per_cell(k);   // mi_knn_search's grid, cell size included
    MI_TRY(search_front_index_and_order(c, b.front, clock, who, ppc, &f));

    FpfhSpfhArgs a{};
    a.q = search_front_queries(b.front, f);
    a.c = search_front_cloud(b.front);
    a.nx = b.nx.p; a.ny = b.ny.p; a.nz = b.nz.p;
    a.k = k; a.max_d2 = max_distance_squared;
    a.keys = b.keys.p; a.packed = b.packed.p; a.count = count ? b.out_count.p : nullptr;
    FpfhSumArgs sa{};
    sa.order = a.q.order; sa.keys = b.keys.p; sa.packed = b.packed.p;
    sa.n = n; sa.k = k;
    sa.fpfh = b.out_fpfh.p; sa.counts = spfh_counts33 ? b.out_counts.p : nullptr;
    // host-side shape checks before the hand-written kernels run: every array they index is as long as the launches assume
    if (!search_front_fits(b.front, f) || !bufs.fits()) {
        set_error("internal: %s buffers shorter than the launch", who);
        return MI_ERR_STATE;
    }
    // with profiling on, K18's time is booked to MI_KERNEL_NN and K19's to MI_KERNEL_MOMENTS (mi_profile_get)
    MI_TRY(search_front_timed_launch(c, b.front, clock, [&] {
        {
            ProfScope p(c, MI_KERNEL_NN);
            const hipError_t e = fpfh_spfh(f.g, a, dist_mode == MI_DIST_FMA, c->stream);
            if (e != hipSuccess) return e;
        }
        ProfScope p(c, MI_KERNEL_MOMENTS);
        return fpfh_sum(sa, c->stream);
    }));

    MI_TRY(bufs.download(c->stream));
    MI_HIP(hipStreamSynchronize(c->stream));
    MI_TRY(clock.mark(6));
    clock.finish();
    return MI_OK;
}

extern "C" int mi_fpfh_features_times(mi_ctx* c, double out_ms[MI_FPFH_STAGES]) { return stage_times("mi_fpfh_features_times", c ? c->fpfh.ms : nullptr, out_ms); }
