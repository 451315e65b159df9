// mi_scan_context, mi_scan_context_search and mi_scan_context_tables behind the C ABI: argument checks, the two tables (stated here, on the
// host, once: the kernel and the restatement both read what mi_scan_context_tables wrote), the reserves of the calls' own buffers in the
// context, the uploads, the launches with their one read-back of the input check, and the download.  The kernels: scan_context_kernels.hip.
#include <hip/hip_runtime.h>

#include <cmath>

#include "context.h"
#include "scan_context_bin.hpp"

using namespace mislam;

static_assert(SC_MAX_RINGS == MI_SCAN_CONTEXT_MAX_RINGS && SC_MAX_SECTORS == MI_SCAN_CONTEXT_MAX_SECTORS && (1 << SC_ROW_BITS) == MI_SCAN_CONTEXT_MAX_ROWS,
              "kernels.h and scan_context_bin.hpp mirror the header's limits");

extern "C" void mi_scan_context_params_default(mi_scan_context_params* p)
{
    if (!p) return;
    *p = mi_scan_context_params{};
    p->rings = 20;
    p->sectors = 60;
    p->max_radius = 80.f;
    p->z_offset = 2.f;
}

// null: the params are usable; otherwise what is wrong with them
static const char* sc_params_fault(const mi_scan_context_params* p)
{
    if (p->rings < 1 || p->rings > MI_SCAN_CONTEXT_MAX_RINGS) return "rings outside [1, 32]";
    if (p->sectors < 1 || p->sectors > MI_SCAN_CONTEXT_MAX_SECTORS) return "sectors outside [1, 64]";
    if (!std::isfinite(p->max_radius) || !(p->max_radius > 0.f)) return "max_radius not finite or not positive";
    if (!std::isfinite(p->z_offset)) return "z_offset not finite";
    return nullptr;
}

// ring_edge2[r] = (max_radius r / rings)^2, the last one max_radius^2 itself; sector_dir[2 j .. 2 j + 1] = (cos, sin)(2 pi j / sectors), the
// axes exact and, for an even number of sectors, the lower half-plane the exact negative of the upper one
static void sc_tables(const mi_scan_context_params* p, double* ring_edge2, double* sector_dir)
{
    const int R = p->rings, S = p->sectors;
    const double mr = (double)p->max_radius;
    for (int r = 0; r < R; r++) {
        const double e = (mr * (double)r) / (double)R;
        ring_edge2[r] = e * e;
    }
    ring_edge2[R] = mr * mr;
    static const double axis[4][2] = {{1.0, 0.0}, {0.0, 1.0}, {-1.0, 0.0}, {0.0, -1.0}};
    for (int j = 0; j < S; j++) {
        if ((4 * j) % S == 0) {
            sector_dir[2 * j] = axis[4 * j / S][0];
            sector_dir[2 * j + 1] = axis[4 * j / S][1];
        } else if (S % 2 == 0 && j >= S / 2) {
            sector_dir[2 * j] = -sector_dir[2 * (j - S / 2)];
            sector_dir[2 * j + 1] = -sector_dir[2 * (j - S / 2) + 1];
        } else {
            const double ang = (2.0 * M_PI * (double)j) / (double)S;
            sector_dir[2 * j] = std::cos(ang);
            sector_dir[2 * j + 1] = std::sin(ang);
        }
    }
}

extern "C" int mi_scan_context_tables(const mi_scan_context_params* params, double* ring_edge2, double* sector_dir)
{
    const char* who = "mi_scan_context_tables";
    if (!params || !ring_edge2 || !sector_dir) { set_error("%s: null params, ring_edge2 or sector_dir", who); return MI_ERR_INVALID_ARG; }
    if (const char* fault = sc_params_fault(params)) { set_error("%s: params: %s", who, fault); return MI_ERR_INVALID_ARG; }
    sc_tables(params, ring_edge2, sector_dir);
    return MI_OK;
}

extern "C" int mi_scan_context(mi_ctx* c, const float* xyz, const int* offsets, int n_scans, const float* centres, const mi_scan_context_params* params,
                               float* desc)
{
    const char* who = "mi_scan_context";
    if (!c) { set_error("%s: null context", who); return MI_ERR_INVALID_ARG; }
    if (!xyz || !offsets || !params || !desc) { set_error("%s: null xyz, offsets, params or desc", who); return MI_ERR_INVALID_ARG; }
    if (n_scans < 1) { set_error("%s: n_scans = %d", who, n_scans); return MI_ERR_INVALID_ARG; }
    if (const char* fault = sc_params_fault(params)) { set_error("%s: params: %s", who, fault); return MI_ERR_INVALID_ARG; }
    if (offsets[0] != 0) { set_error("%s: offsets[0] = %d, not 0", who, offsets[0]); return MI_ERR_INVALID_ARG; }
    int longest = 0;
    for (int s = 0; s < n_scans; s++) {
        if (offsets[s + 1] < offsets[s]) { set_error("%s: offsets descend at index %d (%d after %d)", who, s + 1, offsets[s + 1], offsets[s]); return MI_ERR_INVALID_ARG; }
        if (offsets[s + 1] - offsets[s] > longest) longest = offsets[s + 1] - offsets[s];
    }
    if (centres)
        for (long long e = 0; e < 3LL * n_scans; e++)
            if (!(std::fabs(centres[e]) <= SC_MAX_ABS)) {
                set_error("%s: centres of scan %lld has a non-finite coordinate or one above 1e18 in magnitude", who, e / 3);
                return MI_ERR_INVALID_ARG;
            }
    if (c->distributed()) { set_error("%s: single-GPU contexts only", who); return MI_ERR_STATE; }
    MI_ENTER(c);
    mi_ctx::ScanContextBuffers& b = c->scan_context;
    StageClock clock(c, b.ms);         // mi_scan_context_times

    const int R = params->rings, S = params->sectors;
    const size_t total = (size_t)offsets[n_scans], nb = (size_t)R * (size_t)S, ns = (size_t)n_scans;
    CallBuffers bufs;
    MI_TRY(bufs.need(b.xyz, 3 * total + 1)); MI_TRY(bufs.need(b.offsets, ns + 1)); MI_TRY(bufs.need(b.tables, (size_t)(R + 1 + 2 * S)));
    if (centres) MI_TRY(bufs.need(b.centres, 3 * ns));
    MI_TRY(bufs.need(b.bad, 2)); MI_TRY(bufs.result(b.out_desc, ns * nb, desc));
    MI_TRY(clock.mark(0));

    double tables[MI_SCAN_CONTEXT_MAX_RINGS + 1 + 2 * MI_SCAN_CONTEXT_MAX_SECTORS];
    sc_tables(params, tables, tables + R + 1);
    if (total) MI_TRY(host_to_device(c, b.xyz.p, xyz, sizeof(float) * 3 * total));
    MI_TRY(host_to_device(c, b.offsets.p, offsets, sizeof(int) * (ns + 1)));
    MI_TRY(host_to_device(c, b.tables.p, tables, sizeof(double) * (size_t)(R + 1 + 2 * S)));
    if (centres) MI_TRY(host_to_device(c, b.centres.p, centres, sizeof(float) * 3 * ns));
    MI_TRY(clock.mark(1));

    int slice = SC_SLICE;
    while (((long long)longest + slice - 1) / slice > 65535) slice *= 2;
    ScBinArgs a{};
    a.xyz = b.xyz.p; a.offsets = b.offsets.p; a.centres = centres ? b.centres.p : nullptr;
    a.n_scans = n_scans; a.rings = R; a.sectors = S; a.slice = slice; a.z_offset = params->z_offset;
    a.ring_edge2 = b.tables.p; a.sector_dir = b.tables.p + R + 1;
    a.desc = reinterpret_cast<unsigned int*>(b.out_desc.p); a.bad = b.bad.p;
    // host-side shape checks before the hand-written kernels run: every array they index is as long as the launches assume
    if (!bufs.fits()) {
        set_error("internal: %s buffers shorter than the launch", who);
        return MI_ERR_STATE;
    }
    int bad[2] = {SC_NO_INDEX, SC_NO_INDEX};
    MI_HIP(hipMemcpyAsync(b.bad.p, bad, sizeof bad, hipMemcpyHostToDevice, c->stream));
    MI_HIP(hipMemsetAsync(b.out_desc.p, 0, sizeof(float) * ns * nb, c->stream));
    {
        ProfScope p(c, MI_KERNEL_MOMENTS);
        MI_HIP(sc_bins(a, longest, c->stream));
    }
    MI_HIP(hipMemcpyAsync(bad, b.bad.p, sizeof bad, hipMemcpyDeviceToHost, c->stream));
    MI_HIP(hipStreamSynchronize(c->stream));
    MI_TRY(clock.mark(5));
    if (bad[0] != SC_NO_INDEX) {
        set_error("%s: xyz point %d has a non-finite coordinate or one above 1e18 in magnitude", who, bad[0]);
        return MI_ERR_INVALID_ARG;
    }

    MI_TRY(bufs.download(c->stream));
    MI_HIP(hipStreamSynchronize(c->stream));
    MI_TRY(clock.mark(6));
    clock.finish();
    return MI_OK;
}

extern "C" int mi_scan_context_search(mi_ctx* c, const float* query_desc, int nq, const float* db_desc, int nd, const int* limit,
                                      const mi_scan_context_params* params, int* idx, float* dist, int* shift, float* second_dist)
{
    const char* who = "mi_scan_context_search";
    if (!c) { set_error("%s: null context", who); return MI_ERR_INVALID_ARG; }
    if (!query_desc || !db_desc || !params || !idx || !dist || !shift) { set_error("%s: null query_desc, db_desc, params, idx, dist or shift", who); return MI_ERR_INVALID_ARG; }
    if (nq < 1 || nd < 1) { set_error("%s: empty side (nq = %d, nd = %d)", who, nq, nd); return MI_ERR_INVALID_ARG; }
    if (nd > MI_SCAN_CONTEXT_MAX_ROWS) { set_error("%s: more than %d database rows (nd = %d)", who, MI_SCAN_CONTEXT_MAX_ROWS, nd); return MI_ERR_INVALID_ARG; }
    if (const char* fault = sc_params_fault(params)) { set_error("%s: params: %s", who, fault); return MI_ERR_INVALID_ARG; }
    if (limit)
        for (int i = 0; i < nq; i++)
            if (limit[i] > nd) { set_error("%s: limit of query %d is %d, above nd = %d", who, i, limit[i], nd); return MI_ERR_INVALID_ARG; }
    if (c->distributed()) { set_error("%s: single-GPU contexts only", who); return MI_ERR_STATE; }
    MI_ENTER(c);
    mi_ctx::ScanContextBuffers& b = c->scan_context;
    StageClock clock(c, b.ms);         // mi_scan_context_times

    const int R = params->rings, S = params->sectors;
    const size_t q = (size_t)nq, d = (size_t)nd, nb = (size_t)R * (size_t)S;
    CallBuffers bufs;
    MI_TRY(bufs.need(b.query, q * nb)); MI_TRY(bufs.need(b.db, d * nb)); MI_TRY(bufs.need(b.q_unit, q * nb)); MI_TRY(bufs.need(b.d_unit, d * nb));
    MI_TRY(bufs.need(b.q_mask, q)); MI_TRY(bufs.need(b.d_mask, d)); MI_TRY(bufs.need(b.keys, q)); MI_TRY(bufs.need(b.bad, 2));
    if (limit) MI_TRY(bufs.need(b.limit, q));
    if (second_dist) MI_TRY(bufs.need(b.keys2, q));
    MI_TRY(bufs.result(b.out_idx, q, idx)); MI_TRY(bufs.result(b.out_dist, q, dist)); MI_TRY(bufs.result(b.out_shift, q, shift));
    MI_TRY(bufs.result(b.out_second, q, second_dist));
    MI_TRY(clock.mark(0));

    MI_TRY(host_to_device(c, b.query.p, query_desc, sizeof(float) * q * nb));
    MI_TRY(host_to_device(c, b.db.p, db_desc, sizeof(float) * d * nb));
    if (limit) MI_TRY(host_to_device(c, b.limit.p, limit, sizeof(int) * q));
    MI_TRY(clock.mark(1));

    // host-side shape checks before the hand-written kernels run: every array they index is as long as the launches assume
    if (!bufs.fits()) {
        set_error("internal: %s buffers shorter than the launch", who);
        return MI_ERR_STATE;
    }
    int bad[2] = {SC_NO_INDEX, SC_NO_INDEX};
    MI_HIP(hipMemcpyAsync(b.bad.p, bad, sizeof bad, hipMemcpyHostToDevice, c->stream));
    MI_HIP(sc_normalise(b.query.p, nq, R, S, b.q_unit.p, b.q_mask.p, b.bad.p, c->stream));
    MI_HIP(sc_normalise(b.db.p, nd, R, S, b.d_unit.p, b.d_mask.p, b.bad.p + 1, c->stream));
    MI_HIP(hipMemcpyAsync(bad, b.bad.p, sizeof bad, hipMemcpyDeviceToHost, c->stream));
    MI_HIP(hipStreamSynchronize(c->stream));
    MI_TRY(clock.mark(2));
    for (int side = 0; side < 2; side++)
        if (bad[side] != SC_NO_INDEX) {
            set_error("%s: %s row %d has a negative or non-finite value", who, side == 0 ? "query_desc" : "db_desc", bad[side]);
            return MI_ERR_INVALID_ARG;
        }

    ScSearchArgs a{};
    a.q_unit = b.q_unit.p; a.q_mask = b.q_mask.p; a.nq = nq; a.d_unit = b.d_unit.p; a.d_mask = b.d_mask.p; a.nd = nd;
    a.limit = limit ? b.limit.p : nullptr; a.exclude = nullptr;
    a.rings = R; a.sectors = S; a.chunk_len = sc_chunk_len(nq, nd, c->cu_count); a.keys = b.keys.p;
    MI_HIP(hipMemsetAsync(b.keys.p, 0xff, sizeof(unsigned long long) * q, c->stream));
    if (second_dist) MI_HIP(hipMemsetAsync(b.keys2.p, 0xff, sizeof(unsigned long long) * q, c->stream));
    {
        // with profiling on, the search launches' time is booked to MI_KERNEL_NN (mi_profile_get)
        ProfScope p(c, MI_KERNEL_NN);
        MI_HIP(sc_search(a, c->stream));
    }
    MI_HIP(sc_finish(b.keys.p, nullptr, nq, b.out_idx.p, b.out_dist.p, b.out_shift.p, nullptr, c->stream));
    if (second_dist) {
        // the runner-up: the same search with every query blind to its winner (a query without a winner excludes row -1: none)
        ScSearchArgs a2 = a;
        a2.exclude = b.out_idx.p; a2.keys = b.keys2.p;
        {
            ProfScope p(c, MI_KERNEL_NN);
            MI_HIP(sc_search(a2, c->stream));
        }
        MI_HIP(sc_finish(b.keys.p, b.keys2.p, nq, b.out_idx.p, b.out_dist.p, b.out_shift.p, b.out_second.p, c->stream));
    }
    MI_TRY(clock.mark(5));

    MI_TRY(bufs.download(c->stream));
    MI_HIP(hipStreamSynchronize(c->stream));
    MI_TRY(clock.mark(6));
    clock.finish();
    return MI_OK;
}

extern "C" int mi_scan_context_times(mi_ctx* c, double out_ms[MI_SCAN_CONTEXT_STAGES])
{
    return stage_times("mi_scan_context_times", c ? c->scan_context.ms : nullptr, out_ms);
}
