// mi_mls_smooth behind the C ABI: argument checks, the reserves of the call's own buffers in the context, the search front end
// (search_front.hip: uploads, input check and its one read-back, ONE cell grid over the cloud with cells about one radius long, the curve
// order of the queries -- the cloud's own in self mode, their own where they are a cloud of their own), K50 of mls_kernels.hip over that
// grid and the download of what was asked for.
#include <hip/hip_runtime.h>

#include <cmath>

#include "context.h"
#include "mls_fit.hpp"

using namespace mislam;

static_assert(MLS_QUADRATIC == MI_MLS_QUADRATIC && MLS_PLANE == MI_MLS_PLANE && MLS_UNTOUCHED == MI_MLS_UNTOUCHED, "mls_fit.hpp's verdicts are mi_slam.h's");

extern "C" void mi_mls_params_default(mi_mls_params* p)
{
    if (!p) return;
    *p = mi_mls_params{};
    p->radius = 0.0f;
    p->gauss_scale = 0.0f;
    p->order = 2;
    p->min_neighbours = 3;
    p->dist_mode = MI_DIST_CPU_ROUNDING;
}
static_assert(sizeof(mi_mls_params) == 64, "mi_mls_params is 64 bytes (mi_slam.h)");

extern "C" int mi_mls_smooth(mi_ctx* c, const float* cloud_xyz, int n, const float* query_xyz, int nq, const mi_mls_params* p, float* out_xyz,
                             float* out_normals, float* out_curvature, int* out_neighbours, unsigned char* out_status)
{
    if (!c) { set_error("mi_mls_smooth: null context"); return MI_ERR_INVALID_ARG; }
    if (!cloud_xyz || !p || !out_xyz) { set_error("mi_mls_smooth: null cloud_xyz, params or out_xyz"); return MI_ERR_INVALID_ARG; }
    if (n < 1 || nq < 1) { set_error("mi_mls_smooth: empty cloud or query set (n = %d, nq = %d)", n, nq); return MI_ERR_INVALID_ARG; }
    const bool self = query_xyz == nullptr;
    if (self && nq != n) { set_error("mi_mls_smooth: self mode (query_xyz == NULL) needs nq == n (n = %d, nq = %d)", n, nq); return MI_ERR_INVALID_ARG; }
    if (p->dist_mode != MI_DIST_CPU_ROUNDING && p->dist_mode != MI_DIST_FMA) { set_error("mi_mls_smooth: bad dist_mode %d", p->dist_mode); return MI_ERR_INVALID_ARG; }
    const float r2 = p->radius * p->radius;                                            // one IEEE fp32 multiplication (-ffp-contract=off)
    if (!(std::isfinite(p->radius) && p->radius > 0.f)) { set_error("mi_mls_smooth: radius %g is NaN, infinite or not positive", (double)p->radius); return MI_ERR_INVALID_ARG; }
    if (!std::isfinite(r2)) { set_error("mi_mls_smooth: the square of radius %g is not finite", (double)p->radius); return MI_ERR_INVALID_ARG; }
    if (!(std::isfinite(p->gauss_scale) && p->gauss_scale >= 0.f)) { set_error("mi_mls_smooth: gauss_scale %g is NaN, infinite or negative", (double)p->gauss_scale); return MI_ERR_INVALID_ARG; }
    if (p->order != 1 && p->order != 2) { set_error("mi_mls_smooth: order = %d outside {1, 2}", p->order); return MI_ERR_INVALID_ARG; }
    if (p->min_neighbours < 3) { set_error("mi_mls_smooth: min_neighbours = %d below 3", p->min_neighbours); return MI_ERR_INVALID_ARG; }
    if (c->distributed()) { set_error("mi_mls_smooth: single-GPU contexts only"); return MI_ERR_STATE; }
    MI_ENTER(c);
    mi_ctx::MlsBuffers& b = c->mls;
    StageClock clock(c, b.ms);         // mi_mls_smooth_times

    const size_t rows = (size_t)nq;
    CallBuffers bufs;                  // (in the order of the download)
    MI_TRY(search_front_reserve(b.front, rows, (size_t)n, self));
    MI_TRY(bufs.need(b.out_xyz, 3 * rows, out_xyz)); MI_TRY(bufs.result(b.out_normals, 3 * rows, out_normals));
    MI_TRY(bufs.result(b.out_curvature, rows, out_curvature)); MI_TRY(bufs.result(b.out_neighbours, rows, out_neighbours));
    MI_TRY(bufs.result(b.out_status, rows, out_status));
    MI_TRY(clock.mark(0));

    SearchFront f;
    MI_TRY(search_front_upload_and_check(c, b.front, clock, "mi_mls_smooth", cloud_xyz, n, query_xyz, nq, &f));
    // a cell about one radius long, by the rule of mi_remove_outliers' radius method
    const float ppc = c->tune.knn_points_per_cell > 0.f ? c->tune.knn_points_per_cell : radius_points_per_cell(f.bbox, n, p->radius, c->tune.outlier_radius_cell);
    MI_TRY(search_front_index_and_order(c, b.front, clock, "mi_mls_smooth", ppc, &f));

    // host-side shape checks before the hand-written kernel runs: every array it indexes is as long as the launch assumes
    if (!search_front_fits(b.front, f) || !bufs.fits()) {
        set_error("internal: mi_mls_smooth buffers shorter than the launch");
        return MI_ERR_STATE;
    }
    const double s = p->gauss_scale > 0.f ? (double)p->gauss_scale : (double)p->radius;
    MI_TRY(search_front_timed_launch(c, b.front, clock, [&] {
        MlsArgs a{};
        a.q = search_front_queries(b.front, f);
        a.c = search_front_cloud(b.front);
        a.r2 = r2; a.min_neighbours = p->min_neighbours; a.s2 = s * s;
        a.xyz = b.out_xyz.p; a.normals = out_normals ? b.out_normals.p : nullptr; a.curvature = out_curvature ? b.out_curvature.p : nullptr;
        a.neighbours = out_neighbours ? b.out_neighbours.p : nullptr; a.status = out_status ? b.out_status.p : nullptr;
        return mls_smooth(f.g, a, p->order, p->dist_mode == MI_DIST_FMA, c->stream);
    }));

    MI_TRY(bufs.download(c->stream));
    MI_HIP(hipStreamSynchronize(c->stream));
    MI_TRY(clock.mark(6));
    clock.finish();
    return MI_OK;
}

extern "C" int mi_mls_smooth_times(mi_ctx* c, double out_ms[MI_MLS_STAGES]) { return stage_times("mi_mls_smooth_times", c ? c->mls.ms : nullptr, out_ms); }
