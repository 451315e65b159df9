// mi_iss_keypoints behind the C ABI: argument checks, the reserves of the call's own buffers in the context, the search front end in
// self mode (search_front.hip: upload, input check and its one read-back, ONE cell grid over the cloud with cells about the larger of the
// two radii long, the curve order), K32 and K33 of iss_kernels.hip over that grid, the compaction of K33's flags (outlier_compact, K15's)
// and the download of what was asked for.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "context.h"

using namespace mislam;

extern "C" void mi_iss_params_default(mi_iss_params* p)
{
    if (!p) return;
    *p = mi_iss_params{};
    p->salient_radius = 0.0f;
    p->non_max_radius = 0.0f;
    p->gamma_21 = 0.975f;
    p->gamma_32 = 0.975f;
    p->min_neighbours = 5;
    p->dist_mode = MI_DIST_CPU_ROUNDING;
}
static_assert(sizeof(mi_iss_params) == 64, "mi_iss_params is 64 bytes (mi_slam.h)");

extern "C" int mi_iss_keypoints(mi_ctx* c, const float* cloud_xyz, int n, const mi_iss_params* p, float* out_xyz, int* out_index, int* out_n,
                                unsigned char* is_keypoint, float* saliency, float* eigenvalues, int* neighbours)
{
    if (!c) { set_error("mi_iss_keypoints: null context"); return MI_ERR_INVALID_ARG; }
    if (!cloud_xyz || !p || !out_n) { set_error("mi_iss_keypoints: null cloud_xyz, params or out_n"); return MI_ERR_INVALID_ARG; }
    if (n < 1) { set_error("mi_iss_keypoints: empty cloud (n = %d)", n); return MI_ERR_INVALID_ARG; }
    if (p->dist_mode != MI_DIST_CPU_ROUNDING && p->dist_mode != MI_DIST_FMA) { set_error("mi_iss_keypoints: bad dist_mode %d", p->dist_mode); return MI_ERR_INVALID_ARG; }
    const float r2s = p->salient_radius * p->salient_radius, r2n = p->non_max_radius * p->non_max_radius;   // one IEEE fp32 multiplication each (-ffp-contract=off)
    if (!(std::isfinite(p->salient_radius) && p->salient_radius > 0.f)) { set_error("mi_iss_keypoints: salient_radius %g is NaN, infinite or not positive", (double)p->salient_radius); return MI_ERR_INVALID_ARG; }
    if (!std::isfinite(r2s)) { set_error("mi_iss_keypoints: the square of salient_radius %g is not finite", (double)p->salient_radius); return MI_ERR_INVALID_ARG; }
    if (!(std::isfinite(p->non_max_radius) && p->non_max_radius > 0.f)) { set_error("mi_iss_keypoints: non_max_radius %g is NaN, infinite or not positive", (double)p->non_max_radius); return MI_ERR_INVALID_ARG; }
    if (!std::isfinite(r2n)) { set_error("mi_iss_keypoints: the square of non_max_radius %g is not finite", (double)p->non_max_radius); return MI_ERR_INVALID_ARG; }
    if (!(std::isfinite(p->gamma_21) && p->gamma_21 > 0.f)) { set_error("mi_iss_keypoints: gamma_21 %g is NaN, infinite or not positive", (double)p->gamma_21); return MI_ERR_INVALID_ARG; }
    if (!(std::isfinite(p->gamma_32) && p->gamma_32 > 0.f)) { set_error("mi_iss_keypoints: gamma_32 %g is NaN, infinite or not positive", (double)p->gamma_32); return MI_ERR_INVALID_ARG; }
    const int min_nb = p->min_neighbours;
    if (min_nb < 1) { set_error("mi_iss_keypoints: min_neighbours = %d below 1", min_nb); return MI_ERR_INVALID_ARG; }
    if (c->distributed()) { set_error("mi_iss_keypoints: single-GPU contexts only"); return MI_ERR_STATE; }
    MI_ENTER(c);
    mi_ctx::IssBuffers& b = c->iss;
    StageClock clock(c, b.ms);         // mi_iss_keypoints_times

    const size_t np = (size_t)n;
    const int tiles = outlier_scan_tiles(n);
    CallBuffers bufs;                  // (in the order of the download)
    MI_TRY(search_front_reserve(b.front, np, np, true));
    MI_TRY(bufs.watch(b.front.staging, 3 * np));                                   // the front end's; what the compaction gathers from
    MI_TRY(bufs.need(b.ostate, 1));
    MI_TRY(bufs.need(b.flag, np, is_keypoint)); MI_TRY(bufs.need(b.saliency, np, saliency)); MI_TRY(bufs.need(b.tile_counts, (size_t)tiles));
    MI_TRY(bufs.result(b.eigenvalues, 3 * np, eigenvalues)); MI_TRY(bufs.result(b.neighbours, np, neighbours));
    if (out_xyz) MI_TRY(bufs.need(b.out_xyz, 3 * np));                            // (their rows go once their number is known)
    if (out_index) MI_TRY(bufs.need(b.out_index, np));
    MI_TRY(clock.mark(0));

    SearchFront f;
    MI_TRY(search_front_upload_and_check(c, b.front, clock, "mi_iss_keypoints", cloud_xyz, n, nullptr, n, &f));
    // one cell grid for both walks: a cell about the larger radius long, by the rule of mi_remove_outliers' radius method
    const float ppc = c->tune.knn_points_per_cell > 0.f
                          ? c->tune.knn_points_per_cell
                          : radius_points_per_cell(f.bbox, n, std::max(p->salient_radius, p->non_max_radius), c->tune.outlier_radius_cell);
    MI_TRY(search_front_index_and_order(c, b.front, clock, "mi_iss_keypoints", ppc, &f));

    // host-side shape checks before the hand-written kernels run: every array they index is as long as the launches assume
    if (!search_front_fits(b.front, f) || !bufs.fits()) {
        set_error("internal: mi_iss_keypoints buffers shorter than the launch");
        return MI_ERR_STATE;
    }
    const int fma = p->dist_mode == MI_DIST_FMA;
    MI_TRY(search_front_timed_launch(c, b.front, clock, [&] {
        IssSaliencyArgs a{};
        a.q = search_front_queries(b.front, f);
        a.c = search_front_cloud(b.front);
        a.r2 = r2s; a.min_neighbours = min_nb;
        a.gamma_21 = (double)p->gamma_21; a.gamma_32 = (double)p->gamma_32;
        a.saliency = b.saliency.p; a.eigenvalues = eigenvalues ? b.eigenvalues.p : nullptr; a.neighbours = neighbours ? b.neighbours.p : nullptr;
        return iss_saliency(f.g, a, fma, c->stream);
    }));

    IssSuppressArgs sa{};
    sa.q = search_front_queries(b.front, f);
    sa.r2 = r2n; sa.min_neighbours = min_nb;
    sa.saliency = b.saliency.p; sa.is_keypoint = b.flag.p;
    MI_HIP(iss_suppress(f.g, sa, fma, c->stream));

    MI_HIP(hipMemsetAsync(b.ostate.p, 0, sizeof(OutlierState), c->stream));
    MI_TRY(compact_enqueue(c, b.front, b.flag.p, n, b.tile_counts.p, out_index ? b.out_index.p : nullptr, out_xyz ? b.out_xyz.p : nullptr, b.ostate.p));

    // the state once, with the per-point results; then the keypoints' rows, whose number the state has brought
    MI_TRY(compact_read_state(c, b.ostate.p, 1));
    MI_TRY(bufs.download(c->stream));
    MI_HIP(hipStreamSynchronize(c->stream));
    long long found;
    if (!compact_kept(c, 0, n, &found)) { set_error("internal: mi_iss_keypoints counted %lld keypoints among %d points", found, n); return MI_ERR_STATE; }
    MI_TRY(compact_download(c, found, out_xyz, b.out_xyz.p, out_index, b.out_index.p));
    *out_n = (int)found;
    MI_TRY(clock.mark(6));
    clock.finish();
    return MI_OK;
}

extern "C" int mi_iss_keypoints_times(mi_ctx* c, double out_ms[MI_ISS_STAGES]) { return stage_times("mi_iss_keypoints_times", c ? c->iss.ms : nullptr, out_ms); }
