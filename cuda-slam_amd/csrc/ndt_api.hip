// mi_ndt_constants, mi_ndt_voxels, mi_ndt_register and mi_ndt_system behind the C ABI.  The voxel call is mi_voxel_downsample's front end
// (voxel_front_run, voxel_api.hip) on buffers of its own, then the scatter pass, the per-voxel finish (ndt_kernels.hip) and the download.
// The registration, up to the step kernel's arguments: argument checks, the reserves of the call's own buffers in the context, the uploads, the
// checks of the moving cloud (knn_check_inputs) and of the list (K29) with their read-backs, the table (K30), the moving cloud along its curve
// (morton_order / permute_soa).  The state block, the iterations -- the step of ndt_kernels.hip, then plane_kernels.hip's own reduce and solve --
// in batches of sync_every between host reads of the state, and the results are the pose loop's (pose_loop.hip), which gets the step's launch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>

#include "context.h"
#include "ndt_term.hpp"

using namespace mislam;

namespace {

bool finite_f(float v) { return std::fabs(v) < INFINITY; }      // (false for NaN)

}  // namespace

extern "C" int mi_ndt_constants(float voxel_size, float outlier_ratio, double out[4])
{
    if (!out) { set_error("mi_ndt_constants: null out"); return MI_ERR_INVALID_ARG; }
    if (!finite_f(voxel_size) || !(voxel_size > 0.f)) { set_error("mi_ndt_constants: voxel_size %g is not a positive finite number", (double)voxel_size); return MI_ERR_INVALID_ARG; }
    if (!(outlier_ratio > 0.f && outlier_ratio < 1.f)) { set_error("mi_ndt_constants: outlier_ratio %g is not in (0, 1)", (double)outlier_ratio); return MI_ERR_INVALID_ARG; }
    double k[4];
    ndt_constants((double)voxel_size, (double)outlier_ratio, k);
    for (int i = 0; i < 4; i++)
        if (!std::isfinite(k[i])) { set_error("mi_ndt_constants: voxel_size %g and outlier_ratio %g leave fp64", (double)voxel_size, (double)outlier_ratio); return MI_ERR_INVALID_ARG; }
    for (int i = 0; i < 4; i++) out[i] = k[i];
    return MI_OK;
}

extern "C" int mi_ndt_voxels(mi_ctx* c, const float* xyz, int n, float voxel_size, const float* origin3, int min_points, float eig_ratio, int* out_coord,
                             float* out_mean, float* out_icov6, int* out_n, int* out_count, float* out_cov6, float out_origin[3])
{
    const char* who = "mi_ndt_voxels";
    if (!c) { set_error("%s: null context", who); return MI_ERR_INVALID_ARG; }
    if (!xyz || !out_coord || !out_mean || !out_icov6 || !out_n) { set_error("%s: null xyz, out_coord, out_mean, out_icov6 or out_n", who); return MI_ERR_INVALID_ARG; }
    if (n < 1) { set_error("%s: empty cloud (n = %d)", who, n); return MI_ERR_INVALID_ARG; }
    if (!finite_f(voxel_size) || !(voxel_size > 0.f)) { set_error("%s: voxel_size %g is not a positive finite number", who, (double)voxel_size); return MI_ERR_INVALID_ARG; }
    if (origin3 && !(finite_f(origin3[0]) && finite_f(origin3[1]) && finite_f(origin3[2]))) { set_error("%s: non-finite origin", who); return MI_ERR_INVALID_ARG; }
    if (min_points < 3) { set_error("%s: min_points %d is below 3", who, min_points); return MI_ERR_INVALID_ARG; }
    if (!(eig_ratio > 0.f && eig_ratio <= 1.f)) { set_error("%s: eig_ratio %g is not in (0, 1]", who, (double)eig_ratio); return MI_ERR_INVALID_ARG; }
    if (c->distributed()) { set_error("%s: single-GPU contexts only", who); return MI_ERR_STATE; }
    MI_ENTER(c);
    mi_ctx::NdtBuffers& b = c->ndt;
    StageClock clock(c, b.voxel_ms);

    const size_t np = (size_t)n;
    const size_t sum_tiles = (np + VOX_SUM_TILE - 1) / VOX_SUM_TILE;
    CallBuffers bufs;                  // (every result goes once the number of rows is known)
    MI_TRY(bufs.need(b.q6, 6 * np)); MI_TRY(bufs.need(b.front, 6 * sum_tiles)); MI_TRY(bufs.need(b.back, 6 * sum_tiles)); MI_TRY(bufs.need(b.fix, sum_tiles));
    MI_TRY(bufs.need(b.icov, 6 * np));
    if (out_cov6) MI_TRY(bufs.need(b.cov, 6 * np));
    // the voxel front end's, as the scatter and the finish read them
    MI_TRY(bufs.watch(b.vox.out_xyz, 3 * np)); MI_TRY(bufs.watch(b.vox.out_count, np)); MI_TRY(bufs.watch(b.vox.row_of, np)); MI_TRY(bufs.watch(b.vox.run_start, np + 1));
    NdtScatterArgs a{};
    VoxState* st = nullptr;
    MI_TRY(voxel_front_run(c, who, b.vox, clock, xyz, n, voxel_size, origin3, &a.v, &st));
    const float origin[3] = {st->origin[0], st->origin[1], st->origin[2]};      // (st is the context's scratch: the rows' read-back below lands in it)

    a.front = b.front.p; a.back = b.back.p; a.fix = b.fix.p; a.q6 = b.q6.p;
    // host-side shape checks before the hand-written kernels run: every array they index is as long as the launches assume
    if (!bufs.fits()) {
        set_error("internal: %s buffers shorter than the launch", who);
        return MI_ERR_STATE;
    }
    MI_HIP(ndt_scatter(a, c->stream));
    MI_HIP(ndt_voxel_finish(b.q6.p, b.vox.out_count.p, b.vox.state.p, n, min_points, eig_ratio, b.icov.p, out_cov6 ? b.cov.p : nullptr, c->stream));
    MI_TRY(clock.mark(4));

    MI_HIP(hipMemcpyAsync(&st->rows, &b.vox.state.p->rows, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    MI_HIP(hipStreamSynchronize(c->stream));
    const int rows = st->rows;
    if (rows < 1 || rows > n) { set_error("internal: %s counted %d rows for %d points", who, rows, n); return MI_ERR_STATE; }
    const size_t r = (size_t)rows;
    MI_HIP(hipMemcpyAsync(out_coord, b.vox.out_coord.p, sizeof(int) * 3 * r, hipMemcpyDeviceToHost, c->stream));
    MI_HIP(hipMemcpyAsync(out_mean, b.vox.out_xyz.p, sizeof(float) * 3 * r, hipMemcpyDeviceToHost, c->stream));
    MI_HIP(hipMemcpyAsync(out_icov6, b.icov.p, sizeof(float) * 6 * r, hipMemcpyDeviceToHost, c->stream));
    if (out_count) MI_HIP(hipMemcpyAsync(out_count, b.vox.out_count.p, sizeof(int) * r, hipMemcpyDeviceToHost, c->stream));
    if (out_cov6) MI_HIP(hipMemcpyAsync(out_cov6, b.cov.p, sizeof(float) * 6 * r, hipMemcpyDeviceToHost, c->stream));
    MI_HIP(hipStreamSynchronize(c->stream));
    *out_n = rows;
    if (out_origin)
        for (int k = 0; k < 3; k++) out_origin[k] = origin[k];
    MI_TRY(clock.mark(5));
    clock.finish();
    return MI_OK;
}

extern "C" void mi_ndt_params_default(mi_ndt_params* p)
{
    if (!p) return;
    std::memset(p, 0, sizeof *p);
    p->eps_rotation = 1e-6f;
    p->eps_translation = 1e-6f;
    p->max_iterations = 50;
    p->neighbourhood = 7;
    p->outlier_ratio = 0.55f;
}

namespace {

// what both entry points refuse alike, before the context is touched
int check_arguments(const char* who, mi_ctx* c, const float* before_xyz, int n, const int* vox_coord, const float* vox_mean, const float* vox_icov6, int nv,
                    float voxel_size, const float* origin3, int neighbourhood, float outlier_ratio, const float* T)
{
    if (!c) { set_error("%s: null context", who); return MI_ERR_INVALID_ARG; }
    if (!before_xyz || !vox_coord || !vox_mean || !vox_icov6 || !origin3) { set_error("%s: null before_xyz, vox_coord, vox_mean, vox_icov6 or origin3", who); return MI_ERR_INVALID_ARG; }
    if (n < 1 || nv < 1) { set_error("%s: empty moving cloud or voxel list (n = %d, nv = %d)", who, n, nv); return MI_ERR_INVALID_ARG; }
    if (!finite_f(voxel_size) || !(voxel_size > 0.f)) { set_error("%s: voxel_size %g is not a positive finite number", who, (double)voxel_size); return MI_ERR_INVALID_ARG; }
    if (!(finite_f(origin3[0]) && finite_f(origin3[1]) && finite_f(origin3[2]))) { set_error("%s: non-finite origin", who); return MI_ERR_INVALID_ARG; }
    if (neighbourhood != 1 && neighbourhood != 7 && neighbourhood != 27) { set_error("%s: neighbourhood %d is not 1, 7 or 27", who, neighbourhood); return MI_ERR_INVALID_ARG; }
    if (!(outlier_ratio > 0.f && outlier_ratio < 1.f)) { set_error("%s: outlier_ratio %g is not in (0, 1)", who, (double)outlier_ratio); return MI_ERR_INVALID_ARG; }
    return pose_check_transform(who, T);
}

// Stages 0 - 4 of either call and the state block at pose T: after it the step kernel's arguments are complete and checked against the buffers.
// bufs: the call's list, which brings out_terms (null: not asked for) to the caller behind the step.
int ndt_prepare(mi_ctx* c, const char* who, StageClock& clock, const float* before_xyz, int n, const int* vox_coord, const float* vox_mean,
                const float* vox_icov6, int nv, float voxel_size, const float* origin3, float outlier_ratio, const float* T, bool want_idx,
                unsigned char* out_terms, CallBuffers& bufs, NdtStepArgs* a, PlaneState* h)
{
    mi_ctx::NdtBuffers& b = c->ndt;
    const size_t np = (size_t)n, vp = (size_t)nv;
    const unsigned long long capacity = voxel_table_slots((unsigned long long)nv, 2);
    double constants[4];
    ndt_constants((double)voxel_size, (double)outlier_ratio, constants);
    for (int i = 0; i < 4; i++)
        if (!std::isfinite(constants[i])) { set_error("%s: voxel_size %g and outlier_ratio %g leave fp64", who, (double)voxel_size, (double)outlier_ratio); return MI_ERR_INVALID_ARG; }

    MI_TRY(bufs.need(b.staging, 3 * np));
    MI_TRY(bufs.need(b.ux, np)); MI_TRY(bufs.need(b.uy, np)); MI_TRY(bufs.need(b.uz, np)); MI_TRY(bufs.need(b.qx, np)); MI_TRY(bufs.need(b.qy, np)); MI_TRY(bufs.need(b.qz, np));
    MI_TRY(bufs.need(b.range_lo_hi, 2 * 6 * KNN_RANGE_BLOCKS)); MI_TRY(bufs.need(b.range_bad, 2 * KNN_RANGE_BLOCKS)); MI_TRY(bufs.need(b.kstate, 1)); MI_TRY(bufs.need(b.order, np));
    MI_TRY(bufs.need(b.vcoord, 3 * vp)); MI_TRY(bufs.need(b.vmean, 3 * vp)); MI_TRY(bufs.need(b.vicov, 6 * vp)); MI_TRY(bufs.need(b.mean4, vp)); MI_TRY(bufs.need(b.icov4, 2 * vp));
    MI_TRY(bufs.need(b.mstate, 1)); MI_TRY(bufs.need(b.hkeys, (size_t)capacity)); MI_TRY(bufs.need(b.hvals, (size_t)capacity));
    MI_TRY(pose_loop_reserve(b.loop, n, want_idx));
    MI_TRY(bufs.result(b.out_terms, np, out_terms));
    MortonArgs ma{};
    MI_TRY(morton_args(b.morton, b.ux.p, b.uy.p, b.uz.p, n, b.order.p, &ma));
    MI_TRY(clock.mark(0));

    NdtMapState ms;
    ms.bad_mean = ms.bad_icov = ms.bad_coord = ms.bad_order = NDT_NO_ROW;
    for (int k = 0; k < 3; k++) { ms.cmin[k] = 0x7fffffff; ms.cmax[k] = -0x7fffffff - 1; ms.lo[k] = 0xffffffffu; ms.hi[k] = 0u; }
    ms.with_distribution = 0;
    MI_TRY(host_to_device(c, b.mstate.p, &ms, sizeof ms));
    MI_TRY(host_to_device(c, b.vcoord.p, vox_coord, sizeof(int) * 3 * vp));
    MI_TRY(host_to_device(c, b.vmean.p, vox_mean, sizeof(float) * 3 * vp));
    MI_TRY(host_to_device(c, b.vicov.p, vox_icov6, sizeof(float) * 6 * vp));
    MI_TRY(host_to_device(c, b.staging.p, before_xyz, sizeof(float) * 3 * np));
    MI_HIP(aos_to_soa(b.staging.p, n, n, b.ux.p, b.uy.p, b.uz.p, nullptr, c->stream));
    MI_TRY(clock.mark(1));

    MI_HIP(knn_check_inputs(b.ux.p, b.uy.p, b.uz.p, n, nullptr, nullptr, nullptr, 0, b.range_lo_hi.p, b.range_bad.p, b.kstate.p, c->stream));
    MI_HIP(ndt_check_voxels(b.vcoord.p, b.vmean.p, b.vicov.p, nv, b.mean4.p, b.icov4.p, b.mstate.p, c->stream));
    KnnState* ks = reinterpret_cast<KnnState*>(c->h_scratch);                    // (pinned, 256 bytes: both read-backs fit)
    NdtMapState* hs = reinterpret_cast<NdtMapState*>(c->h_scratch + 16);
    static_assert(sizeof(KnnState) <= 16 * sizeof(float) && sizeof(NdtMapState) <= 48 * sizeof(float), "both states must fit the context's pinned scratch");
    MI_HIP(hipMemcpyAsync(ks, b.kstate.p, sizeof(KnnState), hipMemcpyDeviceToHost, c->stream));
    MI_HIP(hipMemcpyAsync(hs, b.mstate.p, sizeof(NdtMapState), hipMemcpyDeviceToHost, c->stream));
    MI_HIP(hipStreamSynchronize(c->stream));
    MI_TRY(clock.mark(2));
    // everything that can refuse the input is known here, before any output array has been touched
    if (ks->bad_cloud != KNN_NO_POINT) {
        set_error("%s: before_xyz point %d has a non-finite coordinate or one above 1e18 in magnitude", who, ks->bad_cloud);
        return MI_ERR_INVALID_ARG;
    }
    if (hs->bad_mean != NDT_NO_ROW) { set_error("%s: vox_mean row %d has a non-finite entry or one above 1e18 in magnitude", who, hs->bad_mean); return MI_ERR_INVALID_ARG; }
    if (hs->bad_icov != NDT_NO_ROW) { set_error("%s: vox_icov6 row %d has a non-finite entry or one above 1e18 in magnitude", who, hs->bad_icov); return MI_ERR_INVALID_ARG; }
    if (hs->bad_coord != NDT_NO_ROW) { set_error("%s: vox_coord row %d has a coordinate outside [-2^30, 2^30)", who, hs->bad_coord); return MI_ERR_INVALID_ARG; }
    if (hs->bad_order != NDT_NO_ROW) {
        set_error("%s: vox_coord row %d does not come behind row %d in ascending (cz, cy, cx) order", who, hs->bad_order, hs->bad_order - 1);
        return MI_ERR_INVALID_ARG;
    }
    NdtMapView map{};
    const int wide = voxel_table_frame(&map.table, hs->cmin, hs->cmax);
    if (wide >= 0) {
        set_error("%s: the listed voxels span %lld along axis %d (limit 2^20 = %lld)", who, voxel_extent(hs->cmin, hs->cmax, wide), wide, VOXEL_MAX_EXTENT);
        return MI_ERR_INVALID_ARG;
    }
    voxel_table_bind(&map.table, b.hkeys.p, b.hvals.p, capacity);
    map.mean = b.mean4.p; map.icov = b.icov4.p;
    const bool any = hs->with_distribution > 0;
    float centre[3] = {0.f, 0.f, 0.f};       // (no row with a distribution: no term can arise, and the centre is never used)
    for (int k = 0; k < 3 && any; k++) centre[k] = 0.5f * (ndt_key_float(hs->lo[k]) + ndt_key_float(hs->hi[k]));

    MI_HIP(voxel_table_clear(b.hkeys.p, capacity, c->stream));
    if (!bufs.fits()) {
        set_error("internal: %s buffers shorter than the launch", who);
        return MI_ERR_STATE;
    }
    MI_HIP(ndt_hash_build(b.vcoord.p, b.icov4.p, nv, map, b.hkeys.p, b.hvals.p, c->stream));
    MI_TRY(clock.mark(3));

    // the moving cloud along its curve: order[s] = the caller's index of sorted slot s
    MI_HIP(morton_order(ma, c->stream));
    MI_HIP(permute_soa(b.ux.p, b.uy.p, b.uz.p, b.order.p, n, n, b.qx.p, b.qy.p, b.qz.p, c->stream));
    MI_TRY(clock.mark(4));

    MI_TRY(pose_loop_upload_state(c, b.loop, clock, T, centre, h));

    *a = NdtStepArgs{};
    a->state = b.loop.state.p;
    a->bx = b.qx.p; a->by = b.qy.p; a->bz = b.qz.p; a->order = b.order.p;
    a->n = n;
    a->map = map;
    for (int i = 0; i < 3; i++) a->origin[i] = origin3[i];
    a->voxel = voxel_size;
    a->h = constants[2]; a->k = constants[3];
    a->rows = b.loop.rows.p;
    a->idx = want_idx ? b.loop.out_idx.p : nullptr;
    a->terms = out_terms ? b.out_terms.p : nullptr;
    // host-side shape checks before the hand-written kernels run: every array they index is as long as the launches assume
    if (!bufs.fits() || !pose_loop_fits(b.loop, n, want_idx)) {
        set_error("internal: %s buffers shorter than the launch", who);
        return MI_ERR_STATE;
    }
    return MI_OK;
}

}  // namespace

extern "C" int mi_ndt_register(mi_ctx* c, const float* before_xyz, int n, const int* vox_coord, const float* vox_mean, const float* vox_icov6, int nv,
                               float voxel_size, const float origin3[3], const mi_ndt_params* p, const float init_T[16], float out_T[16], int* iterations,
                               float* score, int* stop_reason)
{
    const char* who = "mi_ndt_register";
    if (c && (!p || !out_T)) { set_error("%s: null params or out_T", who); return MI_ERR_INVALID_ARG; }
    MI_TRY(check_arguments(who, c, before_xyz, n, vox_coord, vox_mean, vox_icov6, nv, voxel_size, origin3, p ? p->neighbourhood : 1, p ? p->outlier_ratio : 0.5f, init_T));
    const PoseLoopFields loop{p->eps_rotation, p->eps_translation, p->max_iterations, p->sync_every, p->verbose, "terms"};
    MI_TRY(pose_check_fields(who, loop));
    if (c->distributed()) { set_error("%s: single-GPU contexts only", who); return MI_ERR_STATE; }
    MI_ENTER(c);
    mi_ctx::NdtBuffers& b = c->ndt;
    StageClock clock(c, b.ms);         // mi_ndt_times

    NdtStepArgs a;
    PlaneState h;
    CallBuffers bufs;
    MI_TRY(ndt_prepare(c, who, clock, before_xyz, n, vox_coord, vox_mean, vox_icov6, nv, voxel_size, origin3, p->outlier_ratio, init_T, false, nullptr, bufs, &a, &h));

    MI_TRY(pose_loop_run(c, b.loop, clock, who, n, loop, &h, [&] { return ndt_step(a, p->neighbourhood, c->stream); }));
    return pose_loop_results(clock, h, out_T, iterations, score, stop_reason);
}

extern "C" int mi_ndt_system(mi_ctx* c, const float* before_xyz, int n, const int* vox_coord, const float* vox_mean, const float* vox_icov6, int nv,
                             float voxel_size, const float origin3[3], const float T[16], int neighbourhood, float outlier_ratio, double out_sums[32],
                             float out_centre[3], int* out_idx, unsigned char* out_terms)
{
    const char* who = "mi_ndt_system";
    if (c && !out_sums) { set_error("%s: null out_sums", who); return MI_ERR_INVALID_ARG; }
    MI_TRY(check_arguments(who, c, before_xyz, n, vox_coord, vox_mean, vox_icov6, nv, voxel_size, origin3, neighbourhood, outlier_ratio, T));
    if (c->distributed()) { set_error("%s: single-GPU contexts only", who); return MI_ERR_STATE; }
    MI_ENTER(c);
    mi_ctx::NdtBuffers& b = c->ndt;
    StageClock clock(c, b.ms);         // mi_ndt_times

    NdtStepArgs a;
    PlaneState h;
    CallBuffers bufs;
    MI_TRY(ndt_prepare(c, who, clock, before_xyz, n, vox_coord, vox_mean, vox_icov6, nv, voxel_size, origin3, outlier_ratio, T, out_idx != nullptr, out_terms,
                       bufs, &a, &h));

    MI_TRY(pose_loop_system_run(c, b.loop, clock, n, &h, out_idx, [&] { return ndt_step(a, neighbourhood, c->stream); }));
    MI_TRY(bufs.download(c->stream));
    return pose_loop_system_finish(c, clock, h, out_sums, out_centre);
}

extern "C" int mi_ndt_times(mi_ctx* c, double out_ms[MI_NDT_STAGES]) { return stage_times("mi_ndt_times", c ? c->ndt.ms : nullptr, out_ms); }
