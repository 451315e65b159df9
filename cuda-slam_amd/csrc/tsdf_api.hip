// mi_tsdf_integrate, mi_tsdf_extract, mi_tsdf_mesh, mi_tsdf_raycast and mi_tsdf_times behind the C ABI: argument checks, the host check of a listed map
// (tsdf_ray.hpp), the reserves of the calls' own buffers in the context, the uploads, the launches with their read-backs (the count pass's facts
// and total; the number of voxels; a mesh's vertices and triangles; the blocks and the hits of a ray cast) and the download.  The kernels: tsdf_kernels.hip.  Nothing is written to a caller's array before the last refusal.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>

#include "context.h"
#include "tsdf_cast.hpp"
#include "tsdf_mesh_table.hpp"
#include "tsdf_ray.hpp"

using namespace mislam;

static_assert(TSDF_MAX_HALF_STEPS == MI_TSDF_MAX_HALF_STEPS, "tsdf_ray.hpp mirrors the header's limit");
static_assert(TSDF_RAYCAST_MAX_STEPS == MI_TSDF_RAYCAST_MAX_STEPS, "tsdf_cast.hpp mirrors the header's limit");
static_assert(sizeof(TsdfState) + sizeof(long long) <= 64 * sizeof(float) && sizeof(TsdfState) % sizeof(long long) == 0,
              "the count pass's facts and total must fit the context's pinned scratch");

extern "C" void mi_tsdf_params_default(mi_tsdf_params* p)
{
    if (!p) return;
    *p = mi_tsdf_params{};
    p->min_range = 0.f;
    p->max_range = INFINITY;
    p->max_weight = INFINITY;
}

// the refusals every listed map meets, in both calls; cmin / cmax: its occupied range (nv > 0)
static int tsdf_refuse_map(const char* who, const char* coord_name, const char* tsdf_name, const char* weight_name, const int* coord, const float* tsdf,
                           const float* weight, int nv, int cmin[3], int cmax[3])
{
    int row = 0;
    switch (tsdf_check_map(coord, tsdf, weight, nv, &row, cmin, cmax)) {
    case TSDF_MAP_COORD: set_error("%s: %s row %d has a coordinate outside [-2^30, 2^30)", who, coord_name, row); return MI_ERR_INVALID_ARG;
    case TSDF_MAP_ORDER: set_error("%s: %s row %d is not above row %d in (cz, cy, cx) order", who, coord_name, row, row - 1); return MI_ERR_INVALID_ARG;
    case TSDF_MAP_WEIGHT: set_error("%s: %s row %d is not finite or not positive", who, weight_name, row); return MI_ERR_INVALID_ARG;
    case TSDF_MAP_VALUE: set_error("%s: %s row %d is not finite or outside [-1, 1]", who, tsdf_name, row); return MI_ERR_INVALID_ARG;
    default: return MI_OK;
    }
}

// the frame of a table of the occupied range (nv > 0: every extent is 1 at least)
static int tsdf_refuse_extent(const char* who, const int cmin[3], const int cmax[3], VoxelTableView* t)
{
    const int a = voxel_table_frame(t, cmin, cmax);
    if (a < 0) return MI_OK;
    set_error("%s: the occupied extent along axis %d is %lld voxels, above 2^20", who, a, voxel_extent(cmin, cmax, a));
    return MI_ERR_INVALID_ARG;
}

static bool finite3(const float* v) { return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]); }

extern "C" int mi_tsdf_integrate(mi_ctx* c, const float* scans_xyz, const long long* scan_offsets, int K, const float* scan_T, const float origin3[3],
                                 const mi_tsdf_params* params, const int* in_coord, const float* in_tsdf, const float* in_weight, int nv_in, int* out_coord,
                                 float* out_tsdf, float* out_weight, long long capacity, long long* out_nv)
{
    const char* who = "mi_tsdf_integrate";
    if (!c) { set_error("%s: null context", who); return MI_ERR_INVALID_ARG; }
    if (!scans_xyz || !scan_offsets || !origin3 || !params || !out_nv) { set_error("%s: null scans_xyz, scan_offsets, origin3, params or out_nv", who); return MI_ERR_INVALID_ARG; }
    if (K < 1) { set_error("%s: K = %d", who, K); return MI_ERR_INVALID_ARG; }
    const mi_tsdf_params& p = *params;
    if (!std::isfinite(p.voxel_size) || !(p.voxel_size > 0.f)) { set_error("%s: params: voxel_size not finite or not positive", who); return MI_ERR_INVALID_ARG; }
    if (!std::isfinite(p.truncation) || !((double)p.truncation >= (double)p.voxel_size / 2.0)) { set_error("%s: params: truncation not finite or below voxel_size / 2", who); return MI_ERR_INVALID_ARG; }
    if (!(p.min_range >= 0.f) || !std::isfinite(p.min_range)) { set_error("%s: params: min_range negative or not finite", who); return MI_ERR_INVALID_ARG; }
    if (!(p.max_range > p.min_range)) { set_error("%s: params: max_range not above min_range", who); return MI_ERR_INVALID_ARG; }
    if (!(p.max_weight > 0.f)) { set_error("%s: params: max_weight not positive", who); return MI_ERR_INVALID_ARG; }
    const double half_steps = tsdf_half_steps(p.voxel_size, p.truncation);
    if (half_steps > (double)MI_TSDF_MAX_HALF_STEPS) {
        set_error("%s: params: truncation is %.0f half voxels, above MI_TSDF_MAX_HALF_STEPS = %d", who, half_steps, MI_TSDF_MAX_HALF_STEPS);
        return MI_ERR_INVALID_ARG;
    }
    const int S = (int)half_steps;
    if (scan_offsets[0] != 0) { set_error("%s: scan_offsets[0] = %lld, not 0", who, scan_offsets[0]); return MI_ERR_INVALID_ARG; }
    for (int s = 0; s < K; s++)
        if (scan_offsets[s + 1] < scan_offsets[s]) {
            set_error("%s: scan_offsets descend at index %d (%lld after %lld)", who, s + 1, scan_offsets[s + 1], scan_offsets[s]);
            return MI_ERR_INVALID_ARG;
        }
    const long long rays = scan_offsets[K];
    if (rays == 0) { set_error("%s: scan_offsets end at 0: no point", who); return MI_ERR_INVALID_ARG; }
    if (!finite3(origin3)) { set_error("%s: origin3 not finite", who); return MI_ERR_INVALID_ARG; }
    if (scan_T)
        for (long long e = 0; e < 16LL * K; e++)
            if (!std::isfinite(scan_T[e])) { set_error("%s: scan_T of scan %lld has a non-finite entry (entry %lld)", who, e / 16, e % 16); return MI_ERR_INVALID_ARG; }
    if (nv_in < 0) { set_error("%s: nv_in = %d", who, nv_in); return MI_ERR_INVALID_ARG; }
    if (nv_in > 0 && (!in_coord || !in_tsdf || !in_weight)) { set_error("%s: null in_coord, in_tsdf or in_weight with nv_in = %d", who, nv_in); return MI_ERR_INVALID_ARG; }
    if (capacity < 0) { set_error("%s: capacity = %lld", who, capacity); return MI_ERR_INVALID_ARG; }
    if (capacity > 0 && (!out_coord || !out_tsdf || !out_weight)) { set_error("%s: null out_coord, out_tsdf or out_weight with capacity = %lld", who, capacity); return MI_ERR_INVALID_ARG; }
    if (rays * (long long)(2 * S + 1) + (long long)nv_in >= (1LL << 31)) {
        set_error("%s: %lld rays of %d samples and %d input voxels: 2^31 entries or more", who, rays, 2 * S + 1, nv_in);
        return MI_ERR_INVALID_ARG;
    }
    if (c->distributed()) { set_error("%s: single-GPU contexts only", who); return MI_ERR_STATE; }
    MI_ENTER(c);
    mi_ctx::TsdfBuffers& b = c->tsdf;
    StageClock clock(c, b.ms);         // mi_tsdf_times

    int cmin[3] = {INT_MAX, INT_MAX, INT_MAX}, cmax[3] = {INT_MIN, INT_MIN, INT_MIN};
    MI_TRY(tsdf_refuse_map(who, "in_coord", "in_tsdf", "in_weight", in_coord, in_tsdf, in_weight, nv_in, cmin, cmax));
    MI_TRY(clock.mark(2));

    const size_t nr = (size_t)rays, ns = (size_t)K, nm = (size_t)nv_in;
    CallBuffers bufs;
    MI_TRY(bufs.need(b.xyz, 3 * nr)); MI_TRY(bufs.need(b.offsets, ns + 1));
    if (scan_T) MI_TRY(bufs.need(b.poses, 16 * ns));
    if (nv_in) { MI_TRY(bufs.need(b.in_coord, 3 * nm)); MI_TRY(bufs.need(b.in_tsdf, nm)); MI_TRY(bufs.need(b.in_weight, nm)); }
    MI_TRY(bufs.need(b.count, nr)); MI_TRY(bufs.need(b.tile_sums, (size_t)radius_scan_tiles((int)rays))); MI_TRY(bufs.need(b.sample_off, nr + 1));
    MI_TRY(bufs.need(b.state, 1)); MI_TRY(bufs.need(b.vstate, 1));
    MI_TRY(clock.mark(0));

    MI_TRY(host_to_device(c, b.xyz.p, scans_xyz, sizeof(float) * 3 * nr));
    MI_TRY(host_to_device(c, b.offsets.p, scan_offsets, sizeof(long long) * (ns + 1)));
    if (scan_T) MI_TRY(host_to_device(c, b.poses.p, scan_T, sizeof(float) * 16 * ns));
    if (nv_in) {
        MI_TRY(host_to_device(c, b.in_coord.p, in_coord, sizeof(int) * 3 * nm));
        MI_TRY(host_to_device(c, b.in_tsdf.p, in_tsdf, sizeof(float) * nm));
        MI_TRY(host_to_device(c, b.in_weight.p, in_weight, sizeof(float) * nm));
    }
    MI_TRY(clock.mark(1));

    // host-side shape checks before the hand-written kernels run: every array they index is as long as the launches assume
    if (!bufs.fits()) { set_error("internal: %s buffers shorter than the launch", who); return MI_ERR_STATE; }
    TsdfSampleArgs a{};
    a.xyz = b.xyz.p; a.offsets = b.offsets.p; a.poses = scan_T ? b.poses.p : nullptr; a.n_scans = K; a.rays = (int)rays;
    for (int k = 0; k < 3; k++) a.origin[k] = origin3[k];
    a.voxel = p.voxel_size; a.truncation = p.truncation; a.min_range = p.min_range; a.max_range = p.max_range; a.half_steps = S;
    a.state = b.state.p; a.count = b.count.p;
    const TsdfState start = {TSDF_NO_INDEX, TSDF_NO_INDEX, {INT_MAX, INT_MAX, INT_MAX}, {INT_MIN, INT_MIN, INT_MIN}};
    MI_HIP(hipMemcpyAsync(b.state.p, &start, sizeof start, hipMemcpyHostToDevice, c->stream));
    {
        // with profiling on, the sampling launches' time is booked to MI_KERNEL_NN, the fusion's to MI_KERNEL_MOMENTS (mi_profile_get)
        ProfScope prof(c, MI_KERNEL_NN);
        MI_HIP(tsdf_samples(a, false, c->stream));
    }
    MI_HIP(radius_scan_offsets(b.count.p, (int)rays, b.tile_sums.p, b.sample_off.p, c->stream));
    MI_TRY(clock.mark(3));
    TsdfState* hs = reinterpret_cast<TsdfState*>(c->h_scratch);
    long long* h_total = reinterpret_cast<long long*>(reinterpret_cast<char*>(c->h_scratch) + sizeof(TsdfState));
    MI_HIP(hipMemcpyAsync(hs, b.state.p, sizeof(TsdfState), hipMemcpyDeviceToHost, c->stream));
    MI_HIP(hipMemcpyAsync(h_total, b.sample_off.p + nr, sizeof(long long), hipMemcpyDeviceToHost, c->stream));
    MI_HIP(hipStreamSynchronize(c->stream));
    MI_TRY(clock.mark(2));
    if (hs->bad_point != TSDF_NO_INDEX) {
        set_error("%s: scans_xyz point %d has a non-finite coordinate or one above 1e18 in magnitude", who, hs->bad_point);
        return MI_ERR_INVALID_ARG;
    }
    if (hs->bad_range != TSDF_NO_INDEX) {
        set_error("%s: a sample of scans_xyz point %d has a voxel coordinate outside [-2^30, 2^30)", who, hs->bad_range);
        return MI_ERR_INVALID_ARG;
    }
    const long long samples = *h_total;
    if (samples < 0 || samples > rays * (long long)(2 * S + 1)) { set_error("internal: %s counted %lld samples of %lld rays", who, samples, rays); return MI_ERR_STATE; }
    if (samples > 0)
        for (int k = 0; k < 3; k++) {
            if (hs->cmin[k] < cmin[k]) cmin[k] = hs->cmin[k];
            if (hs->cmax[k] > cmax[k]) cmax[k] = hs->cmax[k];
        }
    const long long entries_ll = samples + (long long)nv_in;
    if (entries_ll == 0) {                   // no input voxel and no surviving sample: the empty map
        *out_nv = 0;
        clock.finish();
        return MI_OK;
    }
    VoxelTableView frame{};                  // (the sort's keys are per axis: only the extent rule is the table's)
    MI_TRY(tsdf_refuse_extent(who, cmin, cmax, &frame));

    const int n = (int)entries_ll;           // (< 2^31: checked above)
    const size_t ne = (size_t)n;
    MI_TRY(bufs.need(b.keys_a, ne)); MI_TRY(bufs.need(b.keys_b, ne)); MI_TRY(bufs.need(b.vals_a, ne)); MI_TRY(bufs.need(b.vals_b, ne));
    MI_TRY(bufs.need(b.axis_keys, 3 * ne)); MI_TRY(bufs.need(b.value, (size_t)samples + 1)); MI_TRY(bufs.need(b.sort_temp, radix_sort_temp_bytes(n) + 16));
    MI_TRY(bufs.need(b.block_heads, (ne + VOX_SCAN_TILE - 1) / VOX_SCAN_TILE)); MI_TRY(bufs.need(b.row_of, ne)); MI_TRY(bufs.need(b.run_start, ne + 1));
    MI_TRY(clock.mark(0));
    if (!bufs.fits()) { set_error("internal: %s entries shorter than the launch", who); return MI_ERR_STATE; }

    a.sample_off = b.sample_off.p; a.base = nv_in; a.entries = ne;
    for (int k = 0; k < 3; k++) a.cmin[k] = cmin[k];
    a.keys = b.keys_a.p; a.axis_keys = b.axis_keys.p; a.vals = b.vals_a.p; a.value = b.value.p;
    if (nv_in) MI_HIP(tsdf_map_keys(b.in_coord.p, nv_in, cmin, ne, b.keys_a.p, b.axis_keys.p, b.vals_a.p, c->stream));
    if (samples > 0) {
        ProfScope prof(c, MI_KERNEL_NN);
        MI_HIP(tsdf_samples(a, true, c->stream));
    }
    MI_TRY(clock.mark(3));

    // least significant axis first; the sort is stable, so the last one leaves (cz, cy, cx) in lexicographic order and, inside a voxel,
    // the entries in the order they were numbered
    auto bits = [&](int k) { return (long long)cmax[k] - cmin[k] + 1 <= 1024 ? 10 : 20; };
    MI_HIP(radix_sort_pairs_u32(b.sort_temp.p, b.keys_a.p, b.keys_b.p, b.vals_a.p, b.vals_b.p, n, bits(0), c->stream));
    MI_HIP(vox_gather_keys(b.axis_keys.p + ne, b.vals_b.p, n, b.keys_a.p, c->stream));
    MI_HIP(radix_sort_pairs_u32(b.sort_temp.p, b.keys_a.p, b.keys_b.p, b.vals_b.p, b.vals_a.p, n, bits(1), c->stream));
    MI_HIP(vox_gather_keys(b.axis_keys.p + 2 * ne, b.vals_a.p, n, b.keys_a.p, c->stream));
    MI_HIP(radix_sort_pairs_u32(b.sort_temp.p, b.keys_a.p, b.keys_b.p, b.vals_a.p, b.vals_b.p, n, bits(2), c->stream));
    VoxArgs v{};
    v.n = n; v.axis_keys = b.axis_keys.p; v.sorted_idx = b.vals_b.p; v.block_heads = b.block_heads.p; v.row_of = b.row_of.p; v.run_start = b.run_start.p;
    v.state = b.vstate.p;
    MI_HIP(vox_rows(v, c->stream));
    MI_TRY(clock.mark(4));
    int* h_rows = reinterpret_cast<int*>(c->h_scratch);
    MI_HIP(hipMemcpyAsync(h_rows, &b.vstate.p->rows, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    MI_HIP(hipStreamSynchronize(c->stream));
    MI_TRY(clock.mark(2));
    const int rows = *h_rows;
    if (rows < 1 || rows > n || rows < nv_in) { set_error("internal: %s found %d voxels among %d entries", who, rows, n); return MI_ERR_STATE; }

    if (capacity > 0 && (long long)rows <= capacity) {
        const size_t nrow = (size_t)rows;
        MI_TRY(bufs.need(b.out_coord, 3 * nrow, out_coord)); MI_TRY(bufs.need(b.out_tsdf, nrow, out_tsdf)); MI_TRY(bufs.need(b.out_weight, nrow, out_weight));
        MI_TRY(clock.mark(0));
        if (!bufs.fits()) { set_error("internal: %s rows shorter than the launch", who); return MI_ERR_STATE; }
        TsdfFuseArgs f{};
        f.sorted_idx = b.vals_b.p; f.run_start = b.run_start.p; f.rows = rows; f.base = nv_in; f.entries = ne; f.axis_keys = b.axis_keys.p;
        for (int k = 0; k < 3; k++) f.cmin[k] = cmin[k];
        f.value = b.value.p; f.in_tsdf = nv_in ? b.in_tsdf.p : nullptr; f.in_weight = nv_in ? b.in_weight.p : nullptr; f.max_weight = p.max_weight;
        f.out_coord = b.out_coord.p; f.out_tsdf = b.out_tsdf.p; f.out_weight = b.out_weight.p;
        {
            ProfScope prof(c, MI_KERNEL_MOMENTS);
            MI_HIP(tsdf_fuse(f, c->stream));
        }
        MI_TRY(clock.mark(5));
        MI_TRY(bufs.download(c->stream));
        MI_HIP(hipStreamSynchronize(c->stream));
        MI_TRY(clock.mark(6));
    }
    *out_nv = rows;
    clock.finish();
    return MI_OK;
}

extern "C" int mi_tsdf_extract(mi_ctx* c, const int* coord, const float* tsdf, const float* weight, int nv, const float origin3[3], float voxel_size,
                               float min_weight, float* out_xyz, float* out_normals, long long capacity, long long* out_n)
{
    const char* who = "mi_tsdf_extract";
    if (!c) { set_error("%s: null context", who); return MI_ERR_INVALID_ARG; }
    if (!origin3 || !out_n) { set_error("%s: null origin3 or out_n", who); return MI_ERR_INVALID_ARG; }
    if (nv < 0) { set_error("%s: nv = %d", who, nv); return MI_ERR_INVALID_ARG; }
    if (nv > 0 && (!coord || !tsdf || !weight)) { set_error("%s: null coord, tsdf or weight with nv = %d", who, nv); return MI_ERR_INVALID_ARG; }
    if (!std::isfinite(voxel_size) || !(voxel_size > 0.f)) { set_error("%s: voxel_size not finite or not positive", who); return MI_ERR_INVALID_ARG; }
    if (!(min_weight > 0.f)) { set_error("%s: min_weight not positive", who); return MI_ERR_INVALID_ARG; }
    if (!finite3(origin3)) { set_error("%s: origin3 not finite", who); return MI_ERR_INVALID_ARG; }
    if (capacity < 0) { set_error("%s: capacity = %lld", who, capacity); return MI_ERR_INVALID_ARG; }
    if (capacity > 0 && !out_xyz) { set_error("%s: null out_xyz with capacity = %lld", who, capacity); return MI_ERR_INVALID_ARG; }
    if (c->distributed()) { set_error("%s: single-GPU contexts only", who); return MI_ERR_STATE; }
    MI_ENTER(c);
    mi_ctx::TsdfBuffers& b = c->tsdf;
    StageClock clock(c, b.ms);         // mi_tsdf_times

    int cmin[3] = {0, 0, 0}, cmax[3] = {0, 0, 0};
    TsdfCrossArgs a{};
    MI_TRY(tsdf_refuse_map(who, "coord", "tsdf", "weight", coord, tsdf, weight, nv, cmin, cmax));
    if (nv > 0) MI_TRY(tsdf_refuse_extent(who, cmin, cmax, &a.table));
    MI_TRY(clock.mark(2));
    if (nv == 0) {                           // the empty map has no surface
        *out_n = 0;
        clock.finish();
        return MI_OK;
    }

    const size_t nm = (size_t)nv, slots = (size_t)voxel_table_slots(nm, 2);
    CallBuffers bufs;
    MI_TRY(bufs.need(b.in_coord, 3 * nm)); MI_TRY(bufs.need(b.in_tsdf, nm)); MI_TRY(bufs.need(b.in_weight, nm));
    MI_TRY(bufs.need(b.hkeys, slots)); MI_TRY(bufs.need(b.hvals, slots));
    MI_TRY(bufs.need(b.count, nm)); MI_TRY(bufs.need(b.tile_sums, (size_t)radius_scan_tiles(nv))); MI_TRY(bufs.need(b.sample_off, nm + 1));
    MI_TRY(clock.mark(0));
    MI_TRY(host_to_device(c, b.in_coord.p, coord, sizeof(int) * 3 * nm));
    MI_TRY(host_to_device(c, b.in_tsdf.p, tsdf, sizeof(float) * nm));
    MI_TRY(host_to_device(c, b.in_weight.p, weight, sizeof(float) * nm));
    MI_TRY(clock.mark(1));

    if (!bufs.fits()) { set_error("internal: %s buffers shorter than the launch", who); return MI_ERR_STATE; }
    a.coord = b.in_coord.p; a.tsdf = b.in_tsdf.p; a.weight = b.in_weight.p; a.nv = nv;
    for (int k = 0; k < 3; k++) a.origin[k] = origin3[k];
    a.voxel = voxel_size; a.min_weight = min_weight;
    voxel_table_bind(&a.table, b.hkeys.p, b.hvals.p, slots);
    a.count = b.count.p;
    MI_HIP(voxel_table_clear(b.hkeys.p, slots, c->stream));
    MI_HIP(tsdf_table(b.in_coord.p, b.in_weight.p, nv, min_weight, a.table, b.hkeys.p, b.hvals.p, c->stream));
    MI_TRY(clock.mark(3));
    {
        // with profiling on, the crossing launches' time is booked to MI_KERNEL_NN (mi_profile_get)
        ProfScope prof(c, MI_KERNEL_NN);
        MI_HIP(tsdf_crossings(a, false, c->stream));
    }
    MI_HIP(radius_scan_offsets(b.count.p, nv, b.tile_sums.p, b.sample_off.p, c->stream));
    long long* h_total = reinterpret_cast<long long*>(c->h_scratch);
    MI_HIP(hipMemcpyAsync(h_total, b.sample_off.p + nm, sizeof(long long), hipMemcpyDeviceToHost, c->stream));
    MI_HIP(hipStreamSynchronize(c->stream));
    MI_TRY(clock.mark(4));
    const long long found = *h_total;
    if (found < 0 || found > 3LL * nv) { set_error("internal: %s counted %lld crossings of %d voxels", who, found, nv); return MI_ERR_STATE; }

    if (capacity > 0 && found > 0 && found <= capacity) {
        const size_t np = (size_t)found;
        MI_TRY(bufs.need(b.out_xyz, 3 * np, out_xyz)); MI_TRY(bufs.result(b.out_normals, 3 * np, out_normals));
        MI_TRY(clock.mark(0));
        if (!bufs.fits()) { set_error("internal: %s lists shorter than the launch", who); return MI_ERR_STATE; }
        a.offsets = b.sample_off.p; a.out_xyz = b.out_xyz.p; a.out_normals = out_normals ? b.out_normals.p : nullptr;
        {
            ProfScope prof(c, MI_KERNEL_NN);
            MI_HIP(tsdf_crossings(a, true, c->stream));
        }
        MI_TRY(clock.mark(5));
        MI_TRY(bufs.download(c->stream));
        MI_HIP(hipStreamSynchronize(c->stream));
        MI_TRY(clock.mark(6));
    }
    *out_n = found;
    clock.finish();
    return MI_OK;
}

extern "C" int mi_tsdf_mesh(mi_ctx* c, const int* coord, const float* tsdf, const float* weight, int nv, const float origin3[3], float voxel_size,
                            float min_weight, float* out_xyz, float* out_normals, long long vertex_capacity, long long* out_nvert, int* out_tri,
                            long long tri_capacity, long long* out_ntri)
{
    const char* who = "mi_tsdf_mesh";
    if (!c) { set_error("%s: null context", who); return MI_ERR_INVALID_ARG; }
    if (!origin3 || !out_nvert || !out_ntri) { set_error("%s: null origin3, out_nvert or out_ntri", who); return MI_ERR_INVALID_ARG; }
    if (nv < 0) { set_error("%s: nv = %d", who, nv); return MI_ERR_INVALID_ARG; }
    if (nv > 0 && (!coord || !tsdf || !weight)) { set_error("%s: null coord, tsdf or weight with nv = %d", who, nv); return MI_ERR_INVALID_ARG; }
    if (!std::isfinite(voxel_size) || !(voxel_size > 0.f)) { set_error("%s: voxel_size not finite or not positive", who); return MI_ERR_INVALID_ARG; }
    if (!(min_weight > 0.f)) { set_error("%s: min_weight not positive", who); return MI_ERR_INVALID_ARG; }
    if (!finite3(origin3)) { set_error("%s: origin3 not finite", who); return MI_ERR_INVALID_ARG; }
    if (vertex_capacity < 0) { set_error("%s: vertex_capacity = %lld", who, vertex_capacity); return MI_ERR_INVALID_ARG; }
    if (tri_capacity < 0) { set_error("%s: tri_capacity = %lld", who, tri_capacity); return MI_ERR_INVALID_ARG; }
    if (vertex_capacity > 0 && !out_xyz) { set_error("%s: null out_xyz with vertex_capacity = %lld", who, vertex_capacity); return MI_ERR_INVALID_ARG; }
    if (tri_capacity > 0 && !out_tri) { set_error("%s: null out_tri with tri_capacity = %lld", who, tri_capacity); return MI_ERR_INVALID_ARG; }
    if (c->distributed()) { set_error("%s: single-GPU contexts only", who); return MI_ERR_STATE; }
    MI_ENTER(c);
    mi_ctx::TsdfBuffers& b = c->tsdf;
    StageClock clock(c, b.ms);         // mi_tsdf_times

    int cmin[3] = {0, 0, 0}, cmax[3] = {0, 0, 0};
    TsdfMeshArgs m{};
    MI_TRY(tsdf_refuse_map(who, "coord", "tsdf", "weight", coord, tsdf, weight, nv, cmin, cmax));
    if (nv > 0) MI_TRY(tsdf_refuse_extent(who, cmin, cmax, &m.table));
    MI_TRY(clock.mark(2));
    if (nv == 0) {                           // the empty map has no surface
        *out_nvert = 0; *out_ntri = 0;
        clock.finish();
        return MI_OK;
    }

    const size_t nm = (size_t)nv, slots = (size_t)voxel_table_slots(nm, 2);
    CallBuffers bufs;
    MI_TRY(bufs.need(b.in_coord, 3 * nm)); MI_TRY(bufs.need(b.in_tsdf, nm)); MI_TRY(bufs.need(b.in_weight, nm));
    MI_TRY(bufs.need(b.hkeys, slots)); MI_TRY(bufs.need(b.hvals, slots));
    MI_TRY(bufs.need(b.count, nm)); MI_TRY(bufs.need(b.tile_sums, (size_t)radius_scan_tiles(nv))); MI_TRY(bufs.need(b.sample_off, nm + 1));
    MI_TRY(bufs.need(b.mesh_case, nm)); MI_TRY(bufs.need(b.mesh_use, nm)); MI_TRY(bufs.need(b.mesh_tris, nm)); MI_TRY(bufs.need(b.tri_off, nm + 1));
    MI_TRY(clock.mark(0));
    MI_TRY(host_to_device(c, b.in_coord.p, coord, sizeof(int) * 3 * nm));
    MI_TRY(host_to_device(c, b.in_tsdf.p, tsdf, sizeof(float) * nm));
    MI_TRY(host_to_device(c, b.in_weight.p, weight, sizeof(float) * nm));
    MI_TRY(clock.mark(1));

    if (!bufs.fits()) { set_error("internal: %s buffers shorter than the launch", who); return MI_ERR_STATE; }
    m.coord = b.in_coord.p; m.tsdf = b.in_tsdf.p; m.weight = b.in_weight.p; m.nv = nv; m.min_weight = min_weight;
    voxel_table_bind(&m.table, b.hkeys.p, b.hvals.p, slots);
    m.cube_case = b.mesh_case.p; m.tri_count = b.mesh_tris.p; m.use = b.mesh_use.p; m.vert_count = b.count.p;
    MI_HIP(voxel_table_clear(b.hkeys.p, slots, c->stream));
    MI_HIP(tsdf_table(b.in_coord.p, b.in_weight.p, nv, min_weight, m.table, b.hkeys.p, b.hvals.p, c->stream));
    MI_TRY(clock.mark(3));
    {
        // with profiling on, the mesh's own launches (K76, K77, K78) are booked to MI_KERNEL_MOMENTS, the shared vertex fill to MI_KERNEL_NN
        ProfScope prof(c, MI_KERNEL_MOMENTS);
        MI_HIP(tsdf_mesh_classify(m, c->stream));
        MI_HIP(tsdf_mesh_edges(m, c->stream));
    }
    // (the two scans share tile_sums: they run one after the other on the stream)
    MI_HIP(radius_scan_offsets(b.count.p, nv, b.tile_sums.p, b.sample_off.p, c->stream));
    MI_HIP(radius_scan_offsets(b.mesh_tris.p, nv, b.tile_sums.p, b.tri_off.p, c->stream));
    long long* h_total = reinterpret_cast<long long*>(c->h_scratch);
    MI_HIP(hipMemcpyAsync(h_total, b.sample_off.p + nm, sizeof(long long), hipMemcpyDeviceToHost, c->stream));
    MI_HIP(hipMemcpyAsync(h_total + 1, b.tri_off.p + nm, sizeof(long long), hipMemcpyDeviceToHost, c->stream));
    MI_HIP(hipStreamSynchronize(c->stream));
    MI_TRY(clock.mark(4));
    const long long nvert = h_total[0], ntri = h_total[1];
    if (nvert < 0 || nvert > 3LL * nv || ntri < 0 || ntri > (long long)TSDF_MESH_MAX_TRIANGLES * nv || (nvert == 0) != (ntri == 0)) {
        set_error("internal: %s counted %lld vertices and %lld triangles of %d voxels", who, nvert, ntri, nv);
        return MI_ERR_STATE;
    }
    if (nvert >= (1LL << 31) || 3 * ntri >= (1LL << 31)) {
        set_error("%s: %lld vertices and %lld triangles: 2^31 vertices or triangle indices, or more", who, nvert, ntri);
        return MI_ERR_INVALID_ARG;
    }

    if (nvert > 0 && nvert <= vertex_capacity && ntri <= tri_capacity) {
        const size_t np = (size_t)nvert, nt = (size_t)ntri;
        MI_TRY(bufs.need(b.out_xyz, 3 * np, out_xyz)); MI_TRY(bufs.result(b.out_normals, 3 * np, out_normals)); MI_TRY(bufs.need(b.out_tri, 3 * nt, out_tri));
        MI_TRY(clock.mark(0));
        if (!bufs.fits()) { set_error("internal: %s lists shorter than the launch", who); return MI_ERR_STATE; }
        TsdfCrossArgs a{};                   // K72's fill, behind K77's masks and their scan
        a.coord = m.coord; a.tsdf = m.tsdf; a.weight = m.weight; a.nv = nv;
        for (int k = 0; k < 3; k++) a.origin[k] = origin3[k];
        a.voxel = voxel_size; a.min_weight = min_weight; a.table = m.table;
        a.count = b.count.p; a.offsets = b.sample_off.p; a.use = b.mesh_use.p;
        a.out_xyz = b.out_xyz.p; a.out_normals = out_normals ? b.out_normals.p : nullptr;
        {
            ProfScope prof(c, MI_KERNEL_NN);
            MI_HIP(tsdf_crossings(a, true, c->stream));
        }
        m.vert_off = b.sample_off.p; m.tri_off = b.tri_off.p; m.out_tri = b.out_tri.p;
        {
            ProfScope prof(c, MI_KERNEL_MOMENTS);
            MI_HIP(tsdf_mesh_triangles(m, c->stream));
        }
        MI_TRY(clock.mark(5));
        MI_TRY(bufs.download(c->stream));
        MI_HIP(hipStreamSynchronize(c->stream));
        MI_TRY(clock.mark(6));
    }
    *out_nvert = nvert; *out_ntri = ntri;
    clock.finish();
    return MI_OK;
}

extern "C" void mi_tsdf_raycast_params_default(mi_tsdf_raycast_params* p)
{
    if (!p) return;
    *p = mi_tsdf_raycast_params{};
    p->min_weight = 1.f;
}

extern "C" int mi_tsdf_raycast(mi_ctx* c, const int* coord, const float* tsdf, const float* weight, int nv, const float origin3[3],
                               const mi_tsdf_raycast_params* params, const float T[16], const float* dirs_xyz, int n, float* out_depth, float* out_xyz,
                               float* out_normals, long long* out_hits)
{
    const char* who = "mi_tsdf_raycast";
    if (!c) { set_error("%s: null context", who); return MI_ERR_INVALID_ARG; }
    if (!origin3 || !params || !dirs_xyz || !out_depth) { set_error("%s: null origin3, params, dirs_xyz or out_depth", who); return MI_ERR_INVALID_ARG; }
    if (n < 1) { set_error("%s: n = %d", who, n); return MI_ERR_INVALID_ARG; }
    if (nv < 0) { set_error("%s: nv = %d", who, nv); return MI_ERR_INVALID_ARG; }
    if (nv > 0 && (!coord || !tsdf || !weight)) { set_error("%s: null coord, tsdf or weight with nv = %d", who, nv); return MI_ERR_INVALID_ARG; }
    const mi_tsdf_raycast_params& p = *params;
    if (!std::isfinite(p.voxel_size) || !(p.voxel_size > 0.f)) { set_error("%s: params: voxel_size not finite or not positive", who); return MI_ERR_INVALID_ARG; }
    if (!(p.min_weight > 0.f)) { set_error("%s: params: min_weight not positive", who); return MI_ERR_INVALID_ARG; }
    if (!(p.min_range >= 0.f) || !std::isfinite(p.min_range)) { set_error("%s: params: min_range negative or not finite", who); return MI_ERR_INVALID_ARG; }
    if (!(p.max_range > p.min_range) || !std::isfinite(p.max_range)) { set_error("%s: params: max_range not finite or not above min_range", who); return MI_ERR_INVALID_ARG; }
    if (p.visit_every_sample != 0 && p.visit_every_sample != 1) { set_error("%s: params: visit_every_sample = %d, neither 0 nor 1", who, p.visit_every_sample); return MI_ERR_INVALID_ARG; }
    const double steps = tsdf_cast_steps(p.voxel_size, p.min_range, p.max_range);
    if (!(steps <= (double)MI_TSDF_RAYCAST_MAX_STEPS)) {
        set_error("%s: params: the range is %.0f samples of half a voxel, above MI_TSDF_RAYCAST_MAX_STEPS = %d", who, steps, MI_TSDF_RAYCAST_MAX_STEPS);
        return MI_ERR_INVALID_ARG;
    }
    if (!finite3(origin3)) { set_error("%s: origin3 not finite", who); return MI_ERR_INVALID_ARG; }
    if (T)
        for (int e = 0; e < 16; e++)
            if (!std::isfinite(T[e])) { set_error("%s: T has a non-finite entry (entry %d)", who, e); return MI_ERR_INVALID_ARG; }
    for (long long e = 0; e < 3LL * n; e++)
        if (!(std::fabs(dirs_xyz[e]) <= TSDF_MAX_ABS)) {
            set_error("%s: dirs_xyz ray %lld has a component that is not finite or above 1e18 in magnitude", who, e / 3);
            return MI_ERR_INVALID_ARG;
        }
    if (c->distributed()) { set_error("%s: single-GPU contexts only", who); return MI_ERR_STATE; }
    MI_ENTER(c);
    mi_ctx::TsdfBuffers& b = c->tsdf;
    StageClock clock(c, b.ms);         // mi_tsdf_times

    int cmin[3] = {0, 0, 0}, cmax[3] = {0, 0, 0};
    TsdfCastArgs a{};
    MI_TRY(tsdf_refuse_map(who, "coord", "tsdf", "weight", coord, tsdf, weight, nv, cmin, cmax));
    if (nv > 0) MI_TRY(tsdf_refuse_extent(who, cmin, cmax, &a.table));
    MI_TRY(clock.mark(2));
    const size_t nr = (size_t)n, nm = (size_t)nv;
    auto every_ray_misses = [&]() {
        for (size_t i = 0; i < nr; i++) out_depth[i] = 0.f;
        for (size_t i = 0; i < 3 * nr; i++) { if (out_xyz) out_xyz[i] = 0.f; if (out_normals) out_normals[i] = 0.f; }
        if (out_hits) *out_hits = 0;
        clock.finish();
        return MI_OK;
    };
    if (nv == 0) return every_ray_misses();  // the empty map

    const size_t slots = (size_t)voxel_table_slots(nm, 2);
    const bool skip = p.visit_every_sample == 0 && tsdf_cast_skip_sound(T, origin3, p.voxel_size, p.max_range);
    CallBuffers bufs;
    MI_TRY(bufs.need(b.in_coord, 3 * nm)); MI_TRY(bufs.need(b.in_tsdf, nm)); MI_TRY(bufs.need(b.in_weight, nm));
    MI_TRY(bufs.need(b.hkeys, slots)); MI_TRY(bufs.need(b.hvals, slots));
    MI_TRY(bufs.need(b.xyz, 3 * nr)); MI_TRY(bufs.need(b.cast_counts, 2));
    if (skip) MI_TRY(bufs.need(b.block_held, slots));
    MI_TRY(bufs.need(b.out_depth, nr, out_depth)); MI_TRY(bufs.result(b.out_xyz, 3 * nr, out_xyz)); MI_TRY(bufs.result(b.out_normals, 3 * nr, out_normals));
    MI_TRY(clock.mark(0));
    MI_TRY(host_to_device(c, b.in_coord.p, coord, sizeof(int) * 3 * nm));
    MI_TRY(host_to_device(c, b.in_tsdf.p, tsdf, sizeof(float) * nm));
    MI_TRY(host_to_device(c, b.in_weight.p, weight, sizeof(float) * nm));
    MI_TRY(host_to_device(c, b.xyz.p, dirs_xyz, sizeof(float) * 3 * nr));
    MI_TRY(clock.mark(1));

    if (!bufs.fits()) { set_error("internal: %s buffers shorter than the launch", who); return MI_ERR_STATE; }
    a.dirs = b.xyz.p; a.n = n; a.has_pose = T ? 1 : 0;
    for (int k = 0; k < 16; k++) a.pose[k] = T ? T[k] : 0.f;
    for (int k = 0; k < 3; k++) a.origin[k] = origin3[k];
    a.voxel = p.voxel_size; a.min_range = p.min_range; a.steps = (int)steps; a.tsdf = b.in_tsdf.p;
    voxel_table_bind(&a.table, b.hkeys.p, b.hvals.p, slots);
    a.out_depth = b.out_depth.p; a.out_xyz = out_xyz ? b.out_xyz.p : nullptr; a.out_normals = out_normals ? b.out_normals.p : nullptr;
    a.hits = b.cast_counts.p + 1;
    MI_HIP(voxel_table_clear(b.hkeys.p, slots, c->stream));
    MI_HIP(hipMemsetAsync(b.cast_counts.p, 0, 2 * sizeof(int), c->stream));
    MI_HIP(tsdf_table(b.in_coord.p, b.in_weight.p, nv, p.min_weight, a.table, b.hkeys.p, b.hvals.p, c->stream));
    MI_TRY(clock.mark(3));

    int* h_count = reinterpret_cast<int*>(c->h_scratch);
    if (skip) {
        // the blocks' frame: the map's range in blocks with one block to spare on every side, for the neighbours K74 marks
        for (int k = 0; k < 3; k++) {
            a.blocks.cmin[k] = (cmin[k] >> TSDF_SKIP_SHIFT) - 1;
            a.blocks.ext[k] = (cmax[k] >> TSDF_SKIP_SHIFT) - (cmin[k] >> TSDF_SKIP_SHIFT) + 3;
        }
        voxel_table_bind(&a.blocks, b.block_held.p, nullptr, slots);
        MI_HIP(voxel_table_clear(b.block_held.p, slots, c->stream));
        MI_HIP(tsdf_blocks(b.in_coord.p, b.in_weight.p, nv, p.min_weight, a.blocks, b.block_held.p, b.cast_counts.p, c->stream));
        MI_HIP(hipMemcpyAsync(h_count, b.cast_counts.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        MI_HIP(hipStreamSynchronize(c->stream));
        const int held = *h_count;
        if (held < 0 || held > nv) { set_error("internal: %s found %d blocks among %d voxels", who, held, nv); return MI_ERR_STATE; }
        if (held == 0) return every_ray_misses();       // no voxel is observed at this min_weight
        const size_t marked = (size_t)voxel_table_slots((unsigned long long)held, 54);
        MI_TRY(bufs.need(b.block_keys, marked));
        if (!bufs.fits()) { set_error("internal: %s block table shorter than the launch", who); return MI_ERR_STATE; }
        MI_HIP(voxel_table_clear(b.block_keys.p, marked, c->stream));
        MI_HIP(tsdf_blocks_dilate(b.block_held.p, (unsigned long long)slots, held, b.block_keys.p, (unsigned long long)marked - 1ull, c->stream));
        voxel_table_bind(&a.blocks, b.block_keys.p, nullptr, marked);
        a.skip = 1;
    }
    MI_TRY(clock.mark(4));
    {
        // with profiling on, the cast launch's time is booked to MI_KERNEL_NN (mi_profile_get)
        ProfScope prof(c, MI_KERNEL_NN);
        MI_HIP(tsdf_cast_rays(a, c->stream));
    }
    MI_TRY(clock.mark(5));
    MI_HIP(hipMemcpyAsync(h_count, b.cast_counts.p + 1, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    MI_TRY(bufs.download(c->stream));
    MI_HIP(hipStreamSynchronize(c->stream));
    MI_TRY(clock.mark(6));
    if (*h_count < 0 || *h_count > n) { set_error("internal: %s counted %d hits of %d rays", who, *h_count, n); return MI_ERR_STATE; }
    if (out_hits) *out_hits = *h_count;
    clock.finish();
    return MI_OK;
}

extern "C" int mi_tsdf_times(mi_ctx* c, double out_ms[MI_TSDF_STAGES]) { return stage_times("mi_tsdf_times", c ? c->tsdf.ms : nullptr, out_ms); }
