// mi_ransac_register and mi_ransac_hypotheses behind the C ABI: argument checks, the correspondences gathered by rank on the host (the
// index array is the host's, one pass over it checks and compacts), the launches of ransac_kernels.hip, the winner's read-back, the
// refinement through mi_kabsch over the inlier flags, and the final pose's flags, count and sum.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "context.h"

using namespace mislam;

extern "C" void mi_ransac_params_default(mi_ransac_params* p)
{
    if (!p) return;
    memset(p, 0, sizeof *p);
    p->hypotheses = 100000;
    p->seed = 0;
    p->max_distance = 0.f;             // the caller must set it
    p->edge_similarity = 0.9f;
    p->refine_iterations = 2;
}

namespace {

struct RansacSetup {
    int C = 0;
    std::vector<int> src_index;
    double e2 = 0.0, max_d2 = 0.0;
};

// the checks both entry points share; nothing has been written or launched when it refuses
int ransac_check(mi_ctx* c, const char* who, const float* src_xyz, int n, const float* tgt_xyz, int m, const int* idx, const mi_ransac_params* p, RansacSetup* out,
                 std::vector<float>* pairs6)
{
    if (!c) { set_error("%s: null context", who); return MI_ERR_INVALID_ARG; }
    if (!src_xyz || !tgt_xyz || !idx || !p) { set_error("%s: null src_xyz, tgt_xyz, idx or params", who); return MI_ERR_INVALID_ARG; }
    if (n < 1 || m < 1) { set_error("%s: empty cloud (n = %d, m = %d)", who, n, m); return MI_ERR_INVALID_ARG; }
    if (p->hypotheses < 1 || p->hypotheses > MI_RANSAC_MAX_HYPOTHESES) { set_error("%s: hypotheses = %d outside [1, %d]", who, p->hypotheses, MI_RANSAC_MAX_HYPOTHESES); return MI_ERR_INVALID_ARG; }
    if (!(p->max_distance > 0.f) || !std::isfinite(p->max_distance)) { set_error("%s: max_distance %g is not a positive finite number", who, (double)p->max_distance); return MI_ERR_INVALID_ARG; }
    if (!(p->edge_similarity >= 0.f && p->edge_similarity < 1.f)) { set_error("%s: edge_similarity %g outside [0, 1)", who, (double)p->edge_similarity); return MI_ERR_INVALID_ARG; }
    if (p->refine_iterations < 0 || p->refine_iterations > MI_RANSAC_MAX_REFINE) { set_error("%s: refine_iterations = %d outside [0, %d]", who, p->refine_iterations, MI_RANSAC_MAX_REFINE); return MI_ERR_INVALID_ARG; }
    if (c->distributed()) { set_error("%s: single-GPU contexts only", who); return MI_ERR_STATE; }
    out->src_index.clear();
    pairs6->clear();
    for (int i = 0; i < n; i++) {
        const int j = idx[i];
        if (j >= m || j < -1) { set_error("%s: idx[%d] = %d is neither -1 nor inside [0, %d)", who, i, j, m); return MI_ERR_INVALID_ARG; }
        if (j < 0) continue;
        out->src_index.push_back(i);
        for (int d = 0; d < 3; d++) pairs6->push_back(src_xyz[3 * (size_t)i + d]);
        for (int d = 0; d < 3; d++) pairs6->push_back(tgt_xyz[3 * (size_t)j + d]);
    }
    out->C = (int)out->src_index.size();
    if (out->C < 3) { set_error("%s: %d correspondences, fewer than 3", who, out->C); return MI_ERR_INVALID_ARG; }
    out->e2 = (double)p->edge_similarity * (double)p->edge_similarity;
    out->max_d2 = (double)p->max_distance * (double)p->max_distance;
    return MI_OK;
}

// reserves, the upload of the correspondences, K23 and K24 over hypotheses first .. first + count - 1 (stages 0 - 3 of the clock)
int ransac_evaluate(mi_ctx* c, StageClock& clock, const RansacSetup& su, const std::vector<float>& pairs6, const mi_ransac_params* p, int first, int count)
{
    mi_ctx::RansacBuffers& b = c->ransac;
    const size_t C = (size_t)su.C, H = (size_t)count;
    MI_TRY(b.pairs6.reserve(6 * C)); MI_TRY(b.src_index.reserve(C)); MI_TRY(b.pose12.reserve(12 * H)); MI_TRY(b.pose.reserve(12));
    MI_TRY(b.triples.reserve(3 * H)); MI_TRY(b.inlier_count.reserve(H)); MI_TRY(b.small.reserve(2)); MI_TRY(b.valid.reserve(H));
    MI_TRY(b.mask.reserve(C)); MI_TRY(b.best.reserve(1)); MI_TRY(b.d2.reserve(C)); MI_TRY(b.sum.reserve(1));
    MI_TRY(clock.mark(0));
    MI_TRY(host_to_device(c, b.pairs6.p, pairs6.data(), sizeof(float) * 6 * C));
    MI_TRY(host_to_device(c, b.src_index.p, su.src_index.data(), sizeof(int) * C));
    MI_TRY(clock.mark(1));
    // host-side shape checks before the hand-written kernels run
    if (b.pairs6.cap < 6 * C || b.src_index.cap < C || b.pose12.cap < 12 * H || b.triples.cap < 3 * H || b.inlier_count.cap < H || b.valid.cap < H || b.mask.cap < C ||
        b.d2.cap < C) {
        set_error("internal: ransac buffers shorter than the launch");
        return MI_ERR_STATE;
    }
    RansacHypArgs ha{};
    ha.pairs6 = b.pairs6.p; ha.src_index = b.src_index.p; ha.C = su.C; ha.seed = p->seed; ha.e2 = su.e2; ha.first = first; ha.count = count;
    ha.triples = b.triples.p; ha.valid = b.valid.p; ha.pose12 = b.pose12.p;
    { ProfScope ps(c, MI_KERNEL_SOLVE); MI_HIP(ransac_hypotheses(ha, c->stream)); }
    MI_TRY(clock.mark(2));
    RansacCountArgs ca{};
    ca.pairs6 = b.pairs6.p; ca.C = su.C; ca.pose12 = b.pose12.p; ca.valid = b.valid.p; ca.count = count; ca.max_d2 = su.max_d2;
    ca.chunk_len = ransac_chunk_len(count, su.C, c->cu_count); ca.inlier_count = b.inlier_count.p;
    MI_HIP(hipMemsetAsync(b.inlier_count.p, 0, sizeof(int) * H, c->stream));
    { ProfScope ps(c, MI_KERNEL_MOMENTS); MI_HIP(ransac_count(ca, c->stream)); }
    MI_TRY(clock.mark(3));
    return MI_OK;
}

// the flags (by rank, into the device mask), the count and the fp64 sum of squared distances of the correspondences under one pose
int ransac_recount(mi_ctx* c, const RansacSetup& su, const float pose[12], int* count, double* sum)
{
    mi_ctx::RansacBuffers& b = c->ransac;
    MI_HIP(hipMemcpyAsync(b.pose.p, pose, sizeof(float) * 12, hipMemcpyHostToDevice, c->stream));
    RansacMaskArgs ma{};
    ma.pairs6 = b.pairs6.p; ma.C = su.C; ma.pose = b.pose.p; ma.max_d2 = su.max_d2; ma.mask = b.mask.p; ma.d2 = b.d2.p;
    MI_HIP(ransac_mask_and_sum(ma, b.small.p + 1, b.sum.p, c->stream));
    MI_HIP(hipMemcpyAsync(count, b.small.p + 1, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    MI_HIP(hipMemcpyAsync(sum, b.sum.p, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    MI_HIP(hipStreamSynchronize(c->stream));
    return MI_OK;
}

}  // namespace

extern "C" int mi_ransac_hypotheses(mi_ctx* c, const float* src_xyz, int n, const float* tgt_xyz, int m, const int* idx, const mi_ransac_params* params, int first,
                                    int count, int* triples, unsigned char* valid, float* pose12, int* inlier_count)
{
    const char* who = "mi_ransac_hypotheses";
    RansacSetup su;
    std::vector<float> pairs6;
    MI_TRY(ransac_check(c, who, src_xyz, n, tgt_xyz, m, idx, params, &su, &pairs6));
    if (first < 0 || count < 1 || (long long)first + count > params->hypotheses) {
        set_error("%s: hypotheses %d .. %d + %d outside [0, %d)", who, first, first, count, params->hypotheses);
        return MI_ERR_INVALID_ARG;
    }
    MI_ENTER(c);
    double ms[8];
    StageClock clock(c, ms);
    MI_TRY(ransac_evaluate(c, clock, su, pairs6, params, first, count));
    mi_ctx::RansacBuffers& b = c->ransac;
    const size_t H = (size_t)count;
    if (triples) MI_HIP(hipMemcpyAsync(triples, b.triples.p, sizeof(int) * 3 * H, hipMemcpyDeviceToHost, c->stream));
    if (valid) MI_HIP(hipMemcpyAsync(valid, b.valid.p, H, hipMemcpyDeviceToHost, c->stream));
    if (pose12) MI_HIP(hipMemcpyAsync(pose12, b.pose12.p, sizeof(float) * 12 * H, hipMemcpyDeviceToHost, c->stream));
    if (inlier_count) MI_HIP(hipMemcpyAsync(inlier_count, b.inlier_count.p, sizeof(int) * H, hipMemcpyDeviceToHost, c->stream));
    MI_HIP(hipStreamSynchronize(c->stream));
    return MI_OK;
}

extern "C" int mi_ransac_register(mi_ctx* c, const float* src_xyz, int n, const float* tgt_xyz, int m, const int* idx, const mi_ransac_params* params,
                                  float out_R9[9], float out_t3[3], int* inliers, float* rmse, int* best_hypothesis, int* valid_hypotheses,
                                  unsigned char* inlier_mask)
{
    const char* who = "mi_ransac_register";
    RansacSetup su;
    std::vector<float> pairs6;
    if (c && (!out_R9 || !out_t3 || !inliers || !rmse || !best_hypothesis || !valid_hypotheses)) { set_error("%s: null output", who); return MI_ERR_INVALID_ARG; }
    MI_TRY(ransac_check(c, who, src_xyz, n, tgt_xyz, m, idx, params, &su, &pairs6));
    std::vector<unsigned char> keep((size_t)n, 0), rank_mask((size_t)su.C, 0);
    float pose[12] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f};
    int count = 0, best_h = -1, nvalid = 0;
    double sum = 0.0;
    {
        MI_ENTER(c);
        mi_ctx::RansacBuffers& b = c->ransac;
        StageClock clock(c, b.ms);         // mi_ransac_register_times
        const int H = params->hypotheses;
        MI_TRY(ransac_evaluate(c, clock, su, pairs6, params, 0, H));
        MI_HIP(hipMemsetAsync(b.best.p, 0, sizeof(unsigned long long), c->stream));
        MI_HIP(hipMemsetAsync(b.small.p, 0, sizeof(int) * 2, c->stream));
        MI_HIP(ransac_argmax(b.valid.p, b.inlier_count.p, H, b.best.p, b.small.p, c->stream));
        unsigned long long best = 0;
        MI_HIP(hipMemcpyAsync(&best, b.best.p, sizeof best, hipMemcpyDeviceToHost, c->stream));
        MI_HIP(hipMemcpyAsync(&nvalid, b.small.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        MI_HIP(hipStreamSynchronize(c->stream));
        if (nvalid > 0) {
            best_h = (int)(0xFFFFFFFFu - (unsigned int)(best & 0xffffffffull));
            if (best_h < 0 || best_h >= H) { set_error("internal: %s winner %d outside [0, %d)", who, best_h, H); return MI_ERR_STATE; }
            MI_HIP(hipMemcpyAsync(pose, b.pose12.p + 12 * (size_t)best_h, sizeof pose, hipMemcpyDeviceToHost, c->stream));
            MI_HIP(hipStreamSynchronize(c->stream));
            MI_TRY(ransac_recount(c, su, pose, &count, &sum));
            MI_HIP(hipMemcpyAsync(rank_mask.data(), b.mask.p, (size_t)su.C, hipMemcpyDeviceToHost, c->stream));
            MI_HIP(hipStreamSynchronize(c->stream));
        }
        MI_TRY(clock.mark(4));
        // refinement: mi_kabsch over the current inliers (its fixed-order fp64 moment sums and solve), a recount; an iteration that leaves
        // fewer than 3 inliers is not taken
        if (nvalid > 0 && params->refine_iterations > 0) {
            std::vector<int> pair_idx((size_t)n);
            for (int i = 0; i < n; i++) pair_idx[i] = idx[i] < 0 ? 0 : idx[i];
            for (int it = 0; it < params->refine_iterations && count >= 3; it++) {
                std::fill(keep.begin(), keep.end(), 0);
                for (int r = 0; r < su.C; r++) keep[su.src_index[r]] = rank_mask[r];
                float trial[12];
                int used = 0;
                const int rc = mi_kabsch(c, src_xyz, n, tgt_xyz, m, pair_idx.data(), keep.data(), trial, trial + 9, &used);
                if (rc != MI_OK) {                         // the message keeps this entry point's name in front
                    const std::string inner = mi_last_error();
                    set_error("%s: refinement pass %d: %s", who, it, inner.c_str());
                    return rc;
                }
                bool finite = true;
                for (float v : trial) finite = finite && std::isfinite(v);
                int trial_count = 0;
                double trial_sum = 0.0;
                if (finite) MI_TRY(ransac_recount(c, su, trial, &trial_count, &trial_sum));
                if (!finite || trial_count < 3) {          // not taken: the device mask goes back to the pose that stays
                    MI_TRY(ransac_recount(c, su, pose, &count, &sum));
                    break;
                }
                memcpy(pose, trial, sizeof pose);
                count = trial_count; sum = trial_sum;
                MI_HIP(hipMemcpyAsync(rank_mask.data(), b.mask.p, (size_t)su.C, hipMemcpyDeviceToHost, c->stream));
                MI_HIP(hipStreamSynchronize(c->stream));
            }
        }
        MI_TRY(clock.mark(5));
        MI_TRY(clock.mark(6));
        clock.finish();
    }
    memcpy(out_R9, pose, sizeof(float) * 9);
    memcpy(out_t3, pose + 9, sizeof(float) * 3);
    *inliers = count;
    *rmse = count > 0 ? (float)std::sqrt(sum / (double)count) : INFINITY;
    *best_hypothesis = best_h;
    *valid_hypotheses = nvalid;
    if (inlier_mask) {
        memset(inlier_mask, 0, (size_t)n);
        for (int r = 0; r < su.C; r++) inlier_mask[su.src_index[r]] = rank_mask[r];
    }
    return MI_OK;
}

extern "C" int mi_ransac_register_times(mi_ctx* c, double out_ms[MI_RANSAC_STAGES]) { return stage_times("mi_ransac_register_times", c ? c->ransac.ms : nullptr, out_ms); }
