// mi_segment_plane and mi_segment_plane_hypotheses behind the C ABI: argument checks, the reserves of the call's own buffers in the
// context, the search front end's upload and input check (search_front.hip; no grid is built), then per round the launches of
// segment_kernels.hip over the remaining points, ransac_argmax and the winner's read-back, the refinement (the sums' read-back, eig3.hpp
// in fp64 on the host, the trial plane's flags and sums in a second set of buffers so that a trial not taken leaves the standing one's in
// place), the labels, and the peel by outlier_compact over the "still without a plane" flags of the whole cloud, which gathers the next
// round's points and their indices.  Read-backs per round: one for the winner and one per plane whose flags are summed (the winner's and
// every refined one): 2 + refine_iterations.  Nothing of the caller's is written before the last round has ended.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "context.h"
#include "eig3.hpp"

using namespace mislam;

namespace {

struct SegmentSetup {
    double T2 = 0.0;
    int has_axis = 0;
    double axis[3] = {0.0, 0.0, 0.0}, cos2 = 0.0;
};

// the checks both entry points share (the distributed context comes behind each one's own); nothing has been written or launched when it refuses
int segment_check(mi_ctx* c, const char* who, const float* cloud_xyz, int n, float thr, int hypotheses, const float* axis3, float cosine, SegmentSetup* su)
{
    if (!c) { set_error("%s: null context", who); return MI_ERR_INVALID_ARG; }
    if (!cloud_xyz) { set_error("%s: null cloud_xyz", who); return MI_ERR_INVALID_ARG; }
    if (n < 3) { set_error("%s: a plane takes 3 points (n = %d)", who, n); return MI_ERR_INVALID_ARG; }
    if (!(std::isfinite(thr) && thr > 0.f)) { set_error("%s: distance_threshold %g is NaN, infinite or not positive", who, (double)thr); return MI_ERR_INVALID_ARG; }
    if (!std::isfinite(thr * thr)) { set_error("%s: the square of distance_threshold %g is not finite", who, (double)thr); return MI_ERR_INVALID_ARG; }
    if (hypotheses < 1 || hypotheses > MI_RANSAC_MAX_HYPOTHESES) { set_error("%s: hypotheses = %d outside [1, %d]", who, hypotheses, MI_RANSAC_MAX_HYPOTHESES); return MI_ERR_INVALID_ARG; }
    su->T2 = (double)thr * (double)thr;
    su->has_axis = axis3 ? 1 : 0;
    if (axis3) {
        bool finite = true, zero = true;
        for (int d = 0; d < 3; d++) { finite = finite && std::isfinite(axis3[d]); zero = zero && axis3[d] == 0.f; su->axis[d] = (double)axis3[d]; }
        if (!finite || zero) { set_error("%s: axis3 (%g, %g, %g) is not finite or zero", who, (double)axis3[0], (double)axis3[1], (double)axis3[2]); return MI_ERR_INVALID_ARG; }
        if (!(cosine >= 0.f && cosine < 1.f)) { set_error("%s: min_axis_cosine %g outside [0, 1)", who, (double)cosine); return MI_ERR_INVALID_ARG; }
        su->cos2 = (double)cosine * (double)cosine;
    }
    return MI_OK;
}

// reserves (stage 0), upload and input check (stages 1, 2), labels = -1, and round 0's remaining points: the whole cloud by rank.
// rows: hypotheses per launch.
int segment_open(mi_ctx* c, StageClock& clock, CallBuffers& bufs, const char* who, const float* cloud_xyz, int n, int rows, int* labels)
{
    mi_ctx::SegmentBuffers& b = c->segment;
    const size_t np = (size_t)n, H = (size_t)rows;
    MI_TRY(search_front_reserve(b.front, np, np, true));
    MI_TRY(bufs.need(b.labels, np, labels)); MI_TRY(bufs.need(b.keep, np)); MI_TRY(bufs.need(b.rem_index, np)); MI_TRY(bufs.need(b.rem_xyz, 3 * np));
    MI_TRY(bufs.need(b.tile_counts, (size_t)outlier_scan_tiles(n))); MI_TRY(bufs.need(b.ostate, 1));
    MI_TRY(bufs.need(b.triples, 3 * H)); MI_TRY(bufs.need(b.valid, H)); MI_TRY(bufs.need(b.plane4, 4 * H)); MI_TRY(bufs.need(b.inlier_count, H));
    MI_TRY(bufs.need(b.nvalid, 1)); MI_TRY(bufs.need(b.best, 1)); MI_TRY(bufs.need(b.plane, 4)); MI_TRY(bufs.need(b.sums, SEGMENT_SUMS));
    for (int k = 0; k < 2; k++) { MI_TRY(bufs.need(b.mask[k], np)); MI_TRY(bufs.need(b.s2[k], np)); }
    MI_TRY(bufs.watch(b.front.staging, 3 * np));
    MI_TRY(clock.mark(0));
    SearchFront f;
    MI_TRY(search_front_upload_and_check(c, b.front, clock, who, cloud_xyz, n, nullptr, n, &f));
    // host-side shape checks before the hand-written kernels run
    if (!bufs.fits()) { set_error("internal: %s buffers shorter than the launch", who); return MI_ERR_STATE; }
    MI_HIP(segment_begin(b.labels.p, b.keep.p, n, c->stream));
    return MI_OK;
}

// the points still without a plane, ascending: their coordinates and indices by rank
int segment_peel(mi_ctx* c, int n)
{
    mi_ctx::SegmentBuffers& b = c->segment;
    OutlierCompactArgs ca{};
    ca.keep = b.keep.p; ca.xyz = b.front.staging.p; ca.n = n; ca.tile_counts = b.tile_counts.p;
    ca.out_index = b.rem_index.p; ca.out_xyz = b.rem_xyz.p; ca.state = b.ostate.p;
    MI_HIP(outlier_compact(ca, c->stream));
    return MI_OK;
}

// K39 and K40 over hypotheses g0 .. g0 + count - 1 on the C remaining points (stages 3 and 4)
int segment_evaluate(mi_ctx* c, StageClock& clock, const SegmentSetup& su, int C, unsigned long long seed, unsigned long long g0, int count)
{
    mi_ctx::SegmentBuffers& b = c->segment;
    SegmentHypArgs ha{};
    ha.rem_xyz = b.rem_xyz.p; ha.rem_index = b.rem_index.p; ha.C = C; ha.seed = seed; ha.g0 = g0; ha.count = count;
    ha.has_axis = su.has_axis; ha.cos2 = su.cos2;
    for (int d = 0; d < 3; d++) ha.axis[d] = su.axis[d];
    ha.triples = b.triples.p; ha.valid = b.valid.p; ha.plane4 = b.plane4.p;
    { ProfScope ps(c, MI_KERNEL_SOLVE); MI_HIP(segment_hypotheses(ha, c->stream)); }
    MI_TRY(clock.mark(3));
    SegmentCountArgs ca{};
    ca.rem_xyz = b.rem_xyz.p; ca.C = C; ca.plane4 = b.plane4.p; ca.valid = b.valid.p; ca.count = count; ca.T2 = su.T2;
    ca.chunk_len = ransac_chunk_len(count, C, c->cu_count); ca.inlier_count = b.inlier_count.p;
    MI_HIP(hipMemsetAsync(b.inlier_count.p, 0, sizeof(int) * (size_t)count, c->stream));
    { ProfScope ps(c, MI_KERNEL_MOMENTS); MI_HIP(segment_count(ca, c->stream)); }
    MI_TRY(clock.mark(4));
    return MI_OK;
}

// the flags and terms (set `set`) of the remaining points under `plane`, and their sums read back: sums[SEGMENT_SUMS]
int segment_sums_under(mi_ctx* c, const SegmentSetup& su, int C, const float plane[4], int set, bool want_scatter, double* sums)
{
    mi_ctx::SegmentBuffers& b = c->segment;
    MI_HIP(hipMemcpyAsync(b.plane.p, plane, sizeof(float) * 4, hipMemcpyHostToDevice, c->stream));
    SegmentMaskArgs ma{};
    ma.rem_xyz = b.rem_xyz.p; ma.C = C; ma.plane = b.plane.p; ma.T2 = su.T2; ma.mask = b.mask[set].p; ma.s2 = b.s2[set].p; ma.sums = b.sums.p;
    MI_HIP(segment_mask_and_sums(ma, want_scatter ? 1 : 0, c->stream));
    double* h = reinterpret_cast<double*>(c->h_scratch);                            // (pinned, 256 bytes)
    MI_HIP(hipMemcpyAsync(h, b.sums.p, sizeof(double) * SEGMENT_SUMS, hipMemcpyDeviceToHost, c->stream));
    MI_HIP(hipStreamSynchronize(c->stream));
    for (int i = 0; i < SEGMENT_SUMS; i++) sums[i] = h[i];
    return MI_OK;
}
static_assert(SEGMENT_SUMS * sizeof(double) <= 64 * sizeof(float), "the sums must fit the context's pinned scratch");

// the least-squares plane of the inliers behind `sums`, turned towards `prev`; false: not finite
bool segment_refit(const double* sums, const float prev[4], float out[4])
{
    const double count = sums[0];
    const double cx = sums[2] / count, cy = sums[3] / count, cz = sums[4] / count;
    const double a6[6] = {sums[5], sums[6], sums[7], sums[8], sums[9], sums[10]};
    double lambda[3], v[9];
    eig3_symmetric<double>(a6, lambda, v);
    double n0 = v[0], n1 = v[3], n2 = v[6];                                         // the column of the smallest eigenvalue
    const double dot = (n0 * (double)prev[0] + n1 * (double)prev[1]) + n2 * (double)prev[2];
    if (dot < 0.0) { n0 = -n0; n1 = -n1; n2 = -n2; }
    const double d = -((n0 * cx + n1 * cy) + n2 * cz);
    out[0] = (float)n0; out[1] = (float)n1; out[2] = (float)n2; out[3] = (float)d;
    return std::isfinite(out[0]) && std::isfinite(out[1]) && std::isfinite(out[2]) && std::isfinite(out[3]);
}

}  // namespace

extern "C" int mi_segment_plane_hypotheses(mi_ctx* c, const float* cloud_xyz, int n, float distance_threshold, int hypotheses, unsigned long long seed,
                                           const float axis3[3], float min_axis_cosine, int first, int count, int* triples, unsigned char* valid,
                                           float* plane4, int* inlier_count)
{
    const char* who = "mi_segment_plane_hypotheses";
    SegmentSetup su;
    MI_TRY(segment_check(c, who, cloud_xyz, n, distance_threshold, hypotheses, axis3, min_axis_cosine, &su));
    if (first < 0 || count < 1 || (long long)first + count > hypotheses) {
        set_error("%s: hypotheses %d .. %d + %d outside [0, %d)", who, first, first, count, hypotheses);
        return MI_ERR_INVALID_ARG;
    }
    if (c->distributed()) { set_error("%s: single-GPU contexts only", who); return MI_ERR_STATE; }
    MI_ENTER(c);
    double ms[8];
    StageClock clock(c, ms);
    CallBuffers bufs;
    MI_TRY(segment_open(c, clock, bufs, who, cloud_xyz, n, count, nullptr));
    MI_TRY(segment_peel(c, n));
    MI_TRY(segment_evaluate(c, clock, su, n, seed, (unsigned long long)first, count));
    mi_ctx::SegmentBuffers& b = c->segment;
    const size_t H = (size_t)count;
    if (triples) MI_HIP(hipMemcpyAsync(triples, b.triples.p, sizeof(int) * 3 * H, hipMemcpyDeviceToHost, c->stream));
    if (valid) MI_HIP(hipMemcpyAsync(valid, b.valid.p, H, hipMemcpyDeviceToHost, c->stream));
    if (plane4) MI_HIP(hipMemcpyAsync(plane4, b.plane4.p, sizeof(float) * 4 * H, hipMemcpyDeviceToHost, c->stream));
    if (inlier_count) MI_HIP(hipMemcpyAsync(inlier_count, b.inlier_count.p, sizeof(int) * H, hipMemcpyDeviceToHost, c->stream));
    MI_HIP(hipStreamSynchronize(c->stream));
    return MI_OK;
}

extern "C" int mi_segment_plane(mi_ctx* c, const float* cloud_xyz, int n, float distance_threshold, int hypotheses, unsigned long long seed,
                                int refine_iterations, int max_planes, int min_inliers, const float axis3[3], float min_axis_cosine, float* planes4,
                                int* n_planes, int* plane_inliers, int* labels, float* rmse, int* winners)
{
    const char* who = "mi_segment_plane";
    SegmentSetup su;
    MI_TRY(segment_check(c, who, cloud_xyz, n, distance_threshold, hypotheses, axis3, min_axis_cosine, &su));
    if (!planes4 || !n_planes) { set_error("%s: null planes4 or n_planes", who); return MI_ERR_INVALID_ARG; }
    if (refine_iterations < 0 || refine_iterations > MI_RANSAC_MAX_REFINE) { set_error("%s: refine_iterations = %d outside [0, %d]", who, refine_iterations, MI_RANSAC_MAX_REFINE); return MI_ERR_INVALID_ARG; }
    if (max_planes < 1 || max_planes > MI_SEGMENT_MAX_PLANES) { set_error("%s: max_planes = %d outside [1, %d]", who, max_planes, MI_SEGMENT_MAX_PLANES); return MI_ERR_INVALID_ARG; }
    if (min_inliers < 3) { set_error("%s: min_inliers = %d below 3", who, min_inliers); return MI_ERR_INVALID_ARG; }
    if (c->distributed()) { set_error("%s: single-GPU contexts only", who); return MI_ERR_STATE; }
    MI_ENTER(c);
    mi_ctx::SegmentBuffers& b = c->segment;
    StageClock clock(c, b.ms);             // mi_segment_plane_times
    CallBuffers bufs;
    MI_TRY(segment_open(c, clock, bufs, who, cloud_xyz, n, hypotheses, labels));

    const int H = hypotheses;
    float out_planes[4 * MI_SEGMENT_MAX_PLANES], out_rmse[MI_SEGMENT_MAX_PLANES];
    int out_count[MI_SEGMENT_MAX_PLANES], out_winner[MI_SEGMENT_MAX_PLANES];
    int found = 0, C = n;
    for (int p = 0; p < max_planes && C >= 3 && C >= min_inliers; p++) {
        MI_TRY(segment_peel(c, n));
        MI_TRY(segment_evaluate(c, clock, su, C, seed, (unsigned long long)p * (unsigned long long)H, H));
        MI_HIP(hipMemsetAsync(b.best.p, 0, sizeof(unsigned long long), c->stream));
        MI_HIP(hipMemsetAsync(b.nvalid.p, 0, sizeof(int), c->stream));
        MI_HIP(ransac_argmax(b.valid.p, b.inlier_count.p, H, b.best.p, b.nvalid.p, c->stream));
        unsigned long long best = 0;
        int nvalid = 0;
        MI_HIP(hipMemcpyAsync(&best, b.best.p, sizeof best, hipMemcpyDeviceToHost, c->stream));
        MI_HIP(hipMemcpyAsync(&nvalid, b.nvalid.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        MI_HIP(hipStreamSynchronize(c->stream));
        MI_TRY(clock.mark(5));
        if (nvalid <= 0) break;
        const int best_h = (int)(0xFFFFFFFFu - (unsigned int)(best & 0xffffffffull));
        const long long won = (long long)(best >> 32);
        if (best_h < 0 || best_h >= H || won > C) { set_error("internal: %s winner %d with %lld of %d points among %d hypotheses", who, best_h, won, C, H); return MI_ERR_STATE; }
        if (won < min_inliers) break;

        float plane[4];
        MI_HIP(hipMemcpyAsync(plane, b.plane4.p + 4 * (size_t)best_h, sizeof plane, hipMemcpyDeviceToHost, c->stream));
        MI_HIP(hipStreamSynchronize(c->stream));
        double sums[SEGMENT_SUMS];
        int set = 0;
        MI_TRY(segment_sums_under(c, su, C, plane, set, refine_iterations > 0, sums));
        if ((long long)sums[0] != won) { set_error("internal: %s counted %lld and then %.0f inliers of one plane", who, won, sums[0]); return MI_ERR_STATE; }
        // refinement: a trial's flags go to the other set, so a trial that is not taken leaves the standing plane's in place
        for (int it = 0; it < refine_iterations && sums[0] >= 3.0; it++) {
            float trial[4];
            double trial_sums[SEGMENT_SUMS];
            if (!segment_refit(sums, plane, trial)) break;
            MI_TRY(segment_sums_under(c, su, C, trial, 1 - set, it + 1 < refine_iterations, trial_sums));
            if (trial_sums[0] < 3.0) break;
            memcpy(plane, trial, sizeof plane);
            memcpy(sums, trial_sums, sizeof sums);
            set = 1 - set;
        }
        const int count = (int)sums[0];
        if (count < 1 || count > C) { set_error("internal: %s plane %d with %d of %d points", who, p, count, C); return MI_ERR_STATE; }
        memcpy(out_planes + 4 * found, plane, sizeof plane);
        out_count[found] = count;
        out_rmse[found] = (float)std::sqrt(sums[1] / (double)count);
        out_winner[found] = best_h;
        MI_HIP(segment_label(b.mask[set].p, b.rem_index.p, C, found, b.labels.p, b.keep.p, c->stream));
        found++;
        C -= count;
        MI_TRY(clock.mark(6));
    }
    MI_TRY(bufs.download(c->stream));
    MI_HIP(hipStreamSynchronize(c->stream));
    memcpy(planes4, out_planes, sizeof(float) * 4 * (size_t)found);
    *n_planes = found;
    if (plane_inliers) memcpy(plane_inliers, out_count, sizeof(int) * (size_t)found);
    if (rmse) memcpy(rmse, out_rmse, sizeof(float) * (size_t)found);
    if (winners) memcpy(winners, out_winner, sizeof(int) * (size_t)found);
    MI_TRY(clock.mark(6));
    clock.finish();
    return MI_OK;
}

extern "C" int mi_segment_plane_times(mi_ctx* c, double out_ms[MI_SEGMENT_STAGES]) { return stage_times("mi_segment_plane_times", c ? c->segment.ms : nullptr, out_ms); }
