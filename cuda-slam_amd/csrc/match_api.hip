// mi_feature_match behind the C ABI: argument checks, the reserves of the call's own buffers in the context, the two uploads, the norms
// with the input check and its one read-back, the forward search and (mutual) the reverse one, the finish kernel, and the download of what
// was asked for.  The kernels: match_kernels.hip.
#include <hip/hip_runtime.h>

#include "context.h"

using namespace mislam;

static_assert(MATCH_MAX_DIM == MI_FEATURE_MAX_DIM, "kernels.h mirrors MI_FEATURE_MAX_DIM");

extern "C" int mi_feature_match(mi_ctx* c, const float* query_feat, int n, const float* target_feat, int m, int dim, int mutual, int* idx, float* d2)
{
    const char* who = "mi_feature_match";
    if (!c) { set_error("%s: null context", who); return MI_ERR_INVALID_ARG; }
    if (!query_feat || !target_feat || !idx) { set_error("%s: null query_feat, target_feat or idx", who); return MI_ERR_INVALID_ARG; }
    if (n < 1 || m < 1) { set_error("%s: empty side (n = %d, m = %d)", who, n, m); return MI_ERR_INVALID_ARG; }
    if (n > MI_FEATURE_MAX_ROWS || m > MI_FEATURE_MAX_ROWS) { set_error("%s: more than %d rows (n = %d, m = %d)", who, MI_FEATURE_MAX_ROWS, n, m); return MI_ERR_INVALID_ARG; }
    if (dim < 1 || dim > MI_FEATURE_MAX_DIM) { set_error("%s: dim = %d outside [1, %d]", who, dim, MI_FEATURE_MAX_DIM); return MI_ERR_INVALID_ARG; }
    if (mutual != 0 && mutual != 1) { set_error("%s: mutual = %d is neither 0 nor 1", who, mutual); return MI_ERR_INVALID_ARG; }
    if (c->distributed()) { set_error("%s: single-GPU contexts only", who); return MI_ERR_STATE; }
    MI_ENTER(c);
    mi_ctx::MatchBuffers& b = c->match;
    StageClock clock(c, b.ms);         // mi_feature_match_times

    const size_t nq = (size_t)n, nt = (size_t)m, d = (size_t)dim;
    CallBuffers bufs;
    MI_TRY(bufs.need(b.query, nq * d)); MI_TRY(bufs.need(b.target, nt * d)); MI_TRY(bufs.need(b.qq, nq)); MI_TRY(bufs.need(b.tt, nt));
    MI_TRY(bufs.need(b.bad, 2)); MI_TRY(bufs.need(b.keys, nq)); MI_TRY(bufs.result(b.out_idx, nq, idx));
    if (mutual) MI_TRY(bufs.need(b.rev_keys, nt));
    MI_TRY(bufs.result(b.out_d2, nq, d2));
    MI_TRY(clock.mark(0));

    MI_TRY(host_to_device(c, b.query.p, query_feat, sizeof(float) * nq * d));
    MI_TRY(host_to_device(c, b.target.p, target_feat, sizeof(float) * nt * d));
    MI_TRY(clock.mark(1));

    int bad[2] = {MATCH_NO_ROW, MATCH_NO_ROW};
    MI_HIP(hipMemcpyAsync(b.bad.p, bad, sizeof bad, hipMemcpyHostToDevice, c->stream));
    MI_HIP(match_norms(b.query.p, n, dim, b.qq.p, b.bad.p, c->stream));
    MI_HIP(match_norms(b.target.p, m, dim, b.tt.p, b.bad.p + 1, c->stream));
    MI_HIP(hipMemcpyAsync(bad, b.bad.p, sizeof bad, hipMemcpyDeviceToHost, c->stream));
    MI_HIP(hipStreamSynchronize(c->stream));
    MI_TRY(clock.mark(2));
    for (int side = 0; side < 2; side++)
        if (bad[side] != MATCH_NO_ROW) {
            set_error("%s: %s row %d has a non-finite component or one above 1e15 in magnitude", who, side == 0 ? "query_feat" : "target_feat", bad[side]);
            return MI_ERR_INVALID_ARG;
        }

    MatchArgs fw{};
    fw.query = b.query.p; fw.target = b.target.p; fw.target_norm = b.tt.p;
    fw.n = n; fw.m = m; fw.dim = dim; fw.chunk_len = match_chunk_len(n, m, c->cu_count); fw.keys = b.keys.p;
    MatchArgs rv{};
    rv.query = b.target.p; rv.target = b.query.p; rv.target_norm = b.qq.p;
    rv.n = m; rv.m = n; rv.dim = dim; rv.chunk_len = match_chunk_len(m, n, c->cu_count); rv.keys = b.rev_keys.p;
    MatchFinishArgs fa{};
    fa.query = b.query.p; fa.target = b.target.p; fa.n = n; fa.m = m; fa.dim = dim;
    fa.keys = b.keys.p; fa.rev_keys = mutual ? b.rev_keys.p : nullptr; fa.idx = b.out_idx.p; fa.d2 = d2 ? b.out_d2.p : nullptr;
    // host-side shape checks before the hand-written kernels run: every array they index is as long as the launches assume
    if (!bufs.fits()) {
        set_error("internal: %s buffers shorter than the launch", who);
        return MI_ERR_STATE;
    }
    // with profiling on, the searches' time is booked to MI_KERNEL_NN (mi_profile_get)
    MI_HIP(hipMemsetAsync(b.keys.p, 0xff, sizeof(unsigned long long) * nq, c->stream));
    if (mutual) MI_HIP(hipMemsetAsync(b.rev_keys.p, 0xff, sizeof(unsigned long long) * nt, c->stream));
    {
        ProfScope p(c, MI_KERNEL_NN);
        MI_HIP(match_search(fw, c->stream));
        if (mutual) MI_HIP(match_search(rv, c->stream));
    }
    MI_HIP(match_finish(fa, c->stream));
    MI_TRY(clock.mark(5));

    MI_TRY(bufs.download(c->stream));
    MI_HIP(hipStreamSynchronize(c->stream));
    MI_TRY(clock.mark(6));
    clock.finish();
    return MI_OK;
}

extern "C" int mi_feature_match_times(mi_ctx* c, double out_ms[MI_MATCH_STAGES]) { return stage_times("mi_feature_match_times", c ? c->match.ms : nullptr, out_ms); }
