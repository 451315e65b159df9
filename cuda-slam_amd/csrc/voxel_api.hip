// mi_voxel_downsample behind the C ABI: argument checks, the call's own buffers in the context, the order of the passes of
// voxel_kernels.hip, the choice between one packed sort and one sort per axis, the two read-backs (the occupied range, the row
// count) and the download; mi_voxel_index is the host statement of the voxel arithmetic the kernels share (voxel_axis, kernels.h).
#include <hip/hip_runtime.h>

#include <cmath>

#include "context.h"

using namespace mislam;

namespace {

constexpr long long VOX_MAX_EXTENT = 1ll << 20;      // voxels per axis between the lowest and the highest occupied one: two radix digits
constexpr long long VOX_PACKED_EXTENT = 1ll << 10;   // up to here on every axis the three coordinates share one 30-bit key

bool finite_f(float v) { return std::fabs(v) < INFINITY; }      // (false for NaN)

}  // namespace

extern "C" int mi_voxel_index(const float p[3], const float origin[3], float voxel_size, int out[3])
{
    if (!p || !origin || !out) { set_error("mi_voxel_index: null argument"); return MI_ERR_INVALID_ARG; }
    if (!finite_f(voxel_size) || !(voxel_size > 0.f)) { set_error("mi_voxel_index: voxel_size %g is not a positive finite number", (double)voxel_size); return MI_ERR_INVALID_ARG; }
    int c[3];
    for (int a = 0; a < 3; a++) {
        if (!finite_f(p[a]) || !finite_f(origin[a])) { set_error("mi_voxel_index: non-finite operand on axis %d", a); return MI_ERR_INVALID_ARG; }
        if (!voxel_axis(p[a], origin[a], voxel_size, &c[a])) {
            set_error("mi_voxel_index: voxel coordinate on axis %d outside [-2^30, 2^30)", a);
            return MI_ERR_INVALID_ARG;
        }
    }
    for (int a = 0; a < 3; a++) out[a] = c[a];
    return MI_OK;
}

int mislam::voxel_front_run(mi_ctx* c, const char* who, mi_ctx::VoxelBuffers& b, StageClock& clock, const float* xyz, int n, float voxel_size,
                            const float* origin3, VoxArgs* args, VoxState** state)
{
    const size_t np = (size_t)n;
    const int scan_tiles = (n + VOX_SCAN_TILE - 1) / VOX_SCAN_TILE, sum_tiles = (n + VOX_SUM_TILE - 1) / VOX_SUM_TILE;
    MI_TRY(b.staging.reserve(3 * np)); MI_TRY(b.x.reserve(np)); MI_TRY(b.y.reserve(np)); MI_TRY(b.z.reserve(np)); MI_TRY(b.pts.reserve(np));
    MI_TRY(b.range_lo_hi.reserve(6 * VOX_RANGE_BLOCKS)); MI_TRY(b.range_bad.reserve(VOX_RANGE_BLOCKS)); MI_TRY(b.state.reserve(1));
    MI_TRY(b.keys_a.reserve(np)); MI_TRY(b.keys_b.reserve(np)); MI_TRY(b.vals_a.reserve(np)); MI_TRY(b.vals_b.reserve(np));
    MI_TRY(b.sort_temp.reserve(radix_sort_temp_bytes(n) + 16));
    MI_TRY(b.block_heads.reserve((size_t)scan_tiles)); MI_TRY(b.row_of.reserve(np)); MI_TRY(b.run_start.reserve(np + 1));
    MI_TRY(b.front.reserve(3 * (size_t)sum_tiles)); MI_TRY(b.back.reserve(3 * (size_t)sum_tiles)); MI_TRY(b.fix.reserve((size_t)sum_tiles));
    MI_TRY(b.out_xyz.reserve(3 * np)); MI_TRY(b.out_count.reserve(np)); MI_TRY(b.out_coord.reserve(3 * np)); MI_TRY(b.voxel_of_point.reserve(np));
    MI_TRY(clock.mark(0));

    MI_TRY(host_to_device(c, b.staging.p, xyz, sizeof(float) * 3 * np));
    MI_HIP(aos_to_soa(b.staging.p, n, n, b.x.p, b.y.p, b.z.p, b.pts.p, c->stream));
    MI_TRY(clock.mark(1));

    VoxArgs& a = *args;
    a = VoxArgs{};
    a.n = n; a.voxel = voxel_size; a.state = b.state.p;
    a.x = b.x.p; a.y = b.y.p; a.z = b.z.p; a.pts = b.pts.p;
    a.range_lo_hi = b.range_lo_hi.p; a.range_bad = b.range_bad.p;
    MI_HIP(vox_range(a, origin3, c->stream));
    VoxState* st = *state = reinterpret_cast<VoxState*>(c->h_scratch);     // (pinned, 256 bytes)
    static_assert(sizeof(VoxState) <= 64 * sizeof(float), "VoxState must fit the context's pinned scratch");
    MI_HIP(hipMemcpyAsync(st, b.state.p, sizeof(VoxState), hipMemcpyDeviceToHost, c->stream));
    MI_HIP(hipStreamSynchronize(c->stream));
    MI_TRY(clock.mark(2));
    // everything that can refuse the cloud is known here, before any output array has been touched
    if (st->bad_index != VOX_NO_POINT) {
        set_error("%s: point %d has a non-finite coordinate", who, st->bad_index);
        return MI_ERR_INVALID_ARG;
    }
    if (st->range_bad != 0) {                // (rare: the host names the first such point; the device only knows that the minimum or the maximum is one)
        int first = -1, cc[3];
        for (int i = 0; i < n && first < 0; i++)
            for (int k = 0; k < 3; k++)
                if (!voxel_axis(xyz[3 * (size_t)i + k], st->origin[k], voxel_size, &cc[k])) { first = i; break; }
        set_error("%s: point %d: voxel coordinate outside [-2^30, 2^30)", who, first);
        return MI_ERR_INVALID_ARG;
    }
    long long extent[3];
    for (int k = 0; k < 3; k++) {
        extent[k] = (long long)st->imax[k] - (long long)st->imin[k] + 1;
        if (extent[k] > VOX_MAX_EXTENT) {
            set_error("%s: the occupied voxels span %lld along axis %d (limit 2^20 = %lld): a larger voxel_size is needed", who, extent[k], k, VOX_MAX_EXTENT);
            return MI_ERR_INVALID_ARG;
        }
    }
    const bool packed = extent[0] <= VOX_PACKED_EXTENT && extent[1] <= VOX_PACKED_EXTENT && extent[2] <= VOX_PACKED_EXTENT;
    if (!packed) { MI_TRY(b.axis_keys.reserve(3 * np)); MI_TRY(clock.mark(0)); }

    a.keys = b.keys_a.p; a.vals = b.vals_a.p; a.axis_keys = packed ? nullptr : b.axis_keys.p;
    MI_HIP(vox_keys(a, c->stream));
    if (packed) {
        MI_HIP(radix_sort_pairs_u32(b.sort_temp.p, b.keys_a.p, b.keys_b.p, b.vals_a.p, b.vals_b.p, n, 30, c->stream));
        a.sorted_keys = b.keys_b.p;
    } else {
        // least significant axis first; the sort is stable, so the last one leaves (cz, cy, cx) in lexicographic order
        auto bits = [&](int k) { return extent[k] <= VOX_PACKED_EXTENT ? 10 : 20; };
        MI_HIP(radix_sort_pairs_u32(b.sort_temp.p, b.keys_a.p, b.keys_b.p, b.vals_a.p, b.vals_b.p, n, bits(0), c->stream));
        MI_HIP(vox_gather_keys(b.axis_keys.p + np, b.vals_b.p, n, b.keys_a.p, c->stream));
        MI_HIP(radix_sort_pairs_u32(b.sort_temp.p, b.keys_a.p, b.keys_b.p, b.vals_b.p, b.vals_a.p, n, bits(1), c->stream));
        MI_HIP(vox_gather_keys(b.axis_keys.p + 2 * np, b.vals_a.p, n, b.keys_a.p, c->stream));
        MI_HIP(radix_sort_pairs_u32(b.sort_temp.p, b.keys_a.p, b.keys_b.p, b.vals_a.p, b.vals_b.p, n, bits(2), c->stream));
    }
    a.sorted_idx = b.vals_b.p;
    MI_TRY(clock.mark(3));

    a.block_heads = b.block_heads.p; a.row_of = b.row_of.p; a.run_start = b.run_start.p;
    a.front = b.front.p; a.back = b.back.p; a.fix = b.fix.p;
    a.out_xyz = b.out_xyz.p; a.out_count = b.out_count.p; a.out_coord = b.out_coord.p; a.voxel_of_point = b.voxel_of_point.p;
    MI_HIP(vox_rows(a, c->stream));
    MI_HIP(vox_sums(a, c->stream));
    MI_TRY(clock.mark(4));

    return MI_OK;
}

extern "C" int mi_voxel_downsample(mi_ctx* c, const float* xyz, int n, float voxel_size, const float* origin3, float* out_xyz, int* out_n,
                                   int* out_count, int* out_coord, int* voxel_of_point)
{
    if (!c) { set_error("mi_voxel_downsample: null context"); return MI_ERR_INVALID_ARG; }
    if (!xyz || !out_xyz || !out_n) { set_error("mi_voxel_downsample: null xyz, out_xyz or out_n"); return MI_ERR_INVALID_ARG; }
    if (n < 1) { set_error("mi_voxel_downsample: empty cloud (n = %d)", n); return MI_ERR_INVALID_ARG; }
    if (!finite_f(voxel_size) || !(voxel_size > 0.f)) { set_error("mi_voxel_downsample: voxel_size %g is not a positive finite number", (double)voxel_size); return MI_ERR_INVALID_ARG; }
    if (origin3 && !(finite_f(origin3[0]) && finite_f(origin3[1]) && finite_f(origin3[2]))) { set_error("mi_voxel_downsample: non-finite origin"); return MI_ERR_INVALID_ARG; }
    if (c->distributed()) { set_error("mi_voxel_downsample: single-GPU contexts only"); return MI_ERR_STATE; }
    MI_ENTER(c);
    mi_ctx::VoxelBuffers& b = c->vox;
    StageClock clock(c, b.ms);         // mi_voxel_downsample_times

    const size_t np = (size_t)n;
    VoxArgs a;
    VoxState* st = nullptr;
    MI_TRY(voxel_front_run(c, "mi_voxel_downsample", b, clock, xyz, n, voxel_size, origin3, &a, &st));

    MI_HIP(hipMemcpyAsync(&st->rows, &b.state.p->rows, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    MI_HIP(hipStreamSynchronize(c->stream));
    const int rows = st->rows;
    if (rows < 1 || rows > n) { set_error("internal: mi_voxel_downsample counted %d rows for %d points", rows, n); return MI_ERR_STATE; }
    MI_HIP(hipMemcpyAsync(out_xyz, b.out_xyz.p, sizeof(float) * 3 * (size_t)rows, hipMemcpyDeviceToHost, c->stream));
    if (out_count) MI_HIP(hipMemcpyAsync(out_count, b.out_count.p, sizeof(int) * (size_t)rows, hipMemcpyDeviceToHost, c->stream));
    if (out_coord) MI_HIP(hipMemcpyAsync(out_coord, b.out_coord.p, sizeof(int) * 3 * (size_t)rows, hipMemcpyDeviceToHost, c->stream));
    if (voxel_of_point) MI_HIP(hipMemcpyAsync(voxel_of_point, b.voxel_of_point.p, sizeof(int) * np, hipMemcpyDeviceToHost, c->stream));
    MI_HIP(hipStreamSynchronize(c->stream));
    *out_n = rows;
    MI_TRY(clock.mark(5));
    clock.finish();
    return MI_OK;
}

extern "C" int mi_voxel_downsample_times(mi_ctx* c, double out_ms[MI_VOXEL_STAGES]) { return stage_times("mi_voxel_downsample_times", c ? c->vox.ms : nullptr, out_ms); }
