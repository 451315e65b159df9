// C ABI, CPD part: rigid CPD driver (replaces CudaCPD, source/cuda-slam/cpdcuda.cu:302-361), its batched form and the test-grade
// E-step / M-step / sigma^2 primitives.  The EM loop is enqueued on one stream; the host reads the state block back
// every `sync_every` iterations only to learn whether the device-side stop rule has fired.  What the entry points enqueue lives in
// cpd_estep.hip and cpd_fgt_api.hip, what they decide on the host in cpd_plan.hpp (cpd_workspace.h: the map).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "cpd_workspace.h"

using namespace mislam;

// return make_pair(scale * rotationMatrix, translationVector)   coherentpointdrift.cpp:123 / cpdcuda.cu:360
static void cpd_state_to_outputs(const CpdState* s, float* out_sR_t, float* out_scale, int* iterations, float* error)
{
    for (int col = 0; col < 3; col++) {
        for (int row = 0; row < 3; row++) out_sR_t[4 * col + row] = s->scale * s->R[3 * col + row];
        out_sR_t[4 * col + 3] = 0.f;
    }
    out_sR_t[12] = s->t[0]; out_sR_t[13] = s->t[1]; out_sR_t[14] = s->t[2]; out_sR_t[15] = 1.f;
    if (out_scale) *out_scale = s->scale;
    *iterations = s->iterations;
    *error = s->error;
}

extern "C" void mi_cpd_params_default(mi_cpd_params* p)
{
    if (!p) return;
    memset(p, 0, sizeof *p);
    p->eps = 1e-3f;            // "convergence-epsilon"  configparser.cpp:244
    p->weight = 0.3f;          // "cpd-weight"           configparser.cpp:238
    p->const_scale = 0;        // "cpd-const-scale"      configparser.cpp:240
    p->max_iterations = -1;    // gpumain.cpp:14 -- NB: runs no iteration, exactly like the reference
    p->tolerance = 1e-3f;      // "cpd-tolerance"        configparser.cpp:242
    p->sigma2_init = 0.f;
    p->sync_every = 0;
    p->verbose = 0;
    p->approximation = MI_CPD_APPROX_NONE;   // the exact P; the reference's parser default is hybrid (configparser.cpp:221-230)
    p->fgt_ratio_of_far_field = 10.0f;       // "fgt-ratio-of-far-field"   configparser.cpp:263
    p->fgt_order_of_truncation = 8;          // "fgt-order-of-truncation"  configparser.cpp:264
}

static int cpd_check(mi_ctx* c, const float* b, int m, const float* a, int n, bool allow_sharded = false)
{
    if (!c) { set_error("CPD: null context"); return MI_ERR_INVALID_ARG; }
    if (!b || !a || m <= 0 || n <= 0) { set_error("CPD: empty or null cloud (m=%d, n=%d)", m, n); return MI_ERR_INVALID_ARG; }
    if (c->world != 1 && !allow_sharded) { set_error("CPD primitives run on single-GPU contexts (mi_cpd_register shards)"); return MI_ERR_STATE; }
    return MI_OK;
}

// What a registration refuses in its parameters whatever the clouds are -- one place for mi_cpd_register and mi_cpd_register_batch, so that
// the batched call refuses exactly what the single call refuses.  `who` names the entry point in the message.
static int cpd_check_params(const mi_cpd_params* params, int world, const char* who)
{
    if (params->approximation < MI_CPD_APPROX_NONE || params->approximation > MI_CPD_APPROX_HYBRID) {
        set_error("%s: unknown approximation %d", who, params->approximation);
        return MI_ERR_INVALID_ARG;
    }
    if (params->approximation != MI_CPD_APPROX_NONE && (params->fgt_order_of_truncation < 1 || params->fgt_order_of_truncation > FGT_MAX_ORDER)) {
        set_error("%s: the FGT modes need 1 <= order of truncation <= %d and >= 2 points per cloud", who, FGT_MAX_ORDER);
        return MI_ERR_INVALID_ARG;
    }
    if (params->estep_mode != MI_ESTEP_DEFAULT && params->estep_mode != MI_ESTEP_CPU_SEQUENTIAL) { set_error("%s: bad estep_mode %d", who, params->estep_mode); return MI_ERR_INVALID_ARG; }
    if (params->estep_mode == MI_ESTEP_CPU_SEQUENTIAL && (world > 1 || params->approximation != MI_CPD_APPROX_NONE)) {
        set_error("%s: MI_ESTEP_CPU_SEQUENTIAL is a single-GPU parity mode of the exact E-step", who);
        return MI_ERR_INVALID_ARG;
    }
    if (params->sigma2_mode != MI_SIGMA2_EXACT && params->sigma2_mode != MI_SIGMA2_CPU_SEQUENTIAL) { set_error("%s: bad sigma2_mode %d", who, params->sigma2_mode); return MI_ERR_INVALID_ARG; }
    return MI_OK;
}
// ... and in the sizes of one pair under those parameters
static int cpd_check_fgt_sizes(const mi_cpd_params* params, long long m, long long n, const char* who)
{
    if (params->approximation != MI_CPD_APPROX_NONE && (m < 2 || n < 2)) {
        set_error("%s: the FGT modes need 1 <= order of truncation <= %d and >= 2 points per cloud (m=%lld, n=%lld)", who, FGT_MAX_ORDER, m, n);
        return MI_ERR_INVALID_ARG;
    }
    return MI_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// the registration loop
// ---------------------------------------------------------------------------------------------------------------
// One EM iteration: the E-step by the route sigma^2 (as the host last read it) asks for, the M-step, the transform.
static int cpd_iteration_enqueue(mi_ctx* c, CpdWorkspace* w, const CpdView& v, const CpdRules& rules, const mi_cpd_params* params)
{
    // (the exact P reads nothing of the host's state block: the pipelined look-ahead enqueues it while a copy into that block is in flight)
    const bool approximated = params->approximation != MI_CPD_APPROX_NONE;
    const float sigma2 = approximated ? w->h_state->sigma2 : 0.f, sigma2_init = approximated ? w->h_state->sigma2_init : 0.f;
    const CpdRouteChoice r = cpd_route(params->approximation, sigma2, sigma2_init);
    if (r.clamped) MI_HIP(cpd_set_sigma2(w->d_state.p, r.sigma2, c->stream));
    if (r.route == CpdRoute::Exact) {
        MI_TRY(cpd_estep_enqueue(c, w, v, params->estep_mode));
    } else if (r.route == CpdRoute::Fgt) {
        MI_TRY(cpd_estep_fgt_enqueue(c, w, v, rules.weight, r.sigma2, sigma2_init, params->fgt_ratio_of_far_field,
                                     params->fgt_order_of_truncation, true));
    } else {
        CpdView vt = v;
        vt.truncate = 1;
        vt.trunc_log = std::log(1e-3f);                // ComputePMatrix(..., true, 1e-3f), :166 / :182-183
        // (MISLAM_CPD_TRUNC_CULL=0 -- round 4's every-pair truncated kernels -- has no sharded form: a sharded registration takes the culled ones)
        if (c->tune.cpd_trunc_cull != 0 || w->queries_sharded) MI_TRY(cpd_estep_trunc_enqueue(c, w, vt));
        else MI_TRY(cpd_estep_enqueue(c, w, vt, params->estep_mode));
    }
    MI_TRY(cpd_mstep_enqueue(c, w, v, rules, 1));
    MI_HIP(cpd_transform(v, w->m_pad, c->stream));
    return MI_OK;
}

// A host check that only PEEKS: the state copy goes behind what is enqueued and an event behind the copy; the caller enqueues more work
// behind the event, then waits for the event alone -- the device does not idle while the host reads.
static int cpd_peek_begin(mi_ctx* c, CpdWorkspace* w)
{
    MI_HIP(hipMemcpyAsync(w->h_state, w->d_state.p, sizeof(CpdState), hipMemcpyDeviceToHost, c->stream));
    MI_HIP(hipEventRecord(c->peek_event, c->stream));
    return MI_OK;
}
static int cpd_peek_wait(mi_ctx* c)
{
    MI_HIP(hipEventSynchronize(c->peek_event));
    return MI_OK;
}

extern "C" int mi_cpd_register(mi_ctx* c, const float* before_xyz, int m_before, const float* after_xyz, int n_after,
                               const mi_cpd_params* params, float out_sR_t[16], float* out_scale, int* iterations, float* error)
{
    MI_TRY(cpd_check(c, before_xyz, m_before, after_xyz, n_after, true));
    if (!params || !out_sR_t || !iterations || !error) { set_error("mi_cpd_register: null argument"); return MI_ERR_INVALID_ARG; }
    if (n_after < c->world) { set_error("mi_cpd_register: %d fixed points cannot be split over %d ranks", n_after, c->world); return MI_ERR_INVALID_ARG; }
    MI_TRY(cpd_check_params(params, c->world, "mi_cpd_register"));
    MI_TRY(cpd_check_fgt_sizes(params, m_before, n_after, "mi_cpd_register"));
    MI_ENTER(c);
    CpdWorkspace* w = nullptr;
    MI_TRY(cpd_workspace(c, &w));
    w->params = *params;
    // every rank is handed both clouds whole (as mi_icp_register) and keeps fixed points [lo, hi) -- mi_shard_range.
    // The FGT modes ("full", and "hybrid" -- the reference parser's default, configparser.cpp:217) cluster the WHOLE fixed cloud and
    // their E-step is O((N + M) K) -- milliseconds where the exact one takes seconds -- so on a multi-rank context they run
    // REPLICATED: every rank keeps both clouds whole and does the same arithmetic in the same order (the same bits everywhere),
    // no collective at all.  The exact P shards.
    int lo = 0, hi = n_after;
    w->replicated = c->world > 1 && params->approximation != MI_CPD_APPROX_NONE;
    w->queries_sharded = w->replicated && c->tune.fgt_shard_queries != 0 && cpd_trunc_tiles(m_before) >= c->world && cpd_trunc_tiles(n_after) >= c->world;
    if (w->queries_sharded) {
        (void)mi_shard_range(n_after, c->rank, c->world, &w->a_lo, &w->a_hi);
        (void)mi_shard_range(m_before, c->rank, c->world, &w->m_lo, &w->m_hi);
    }
    if (c->world > 1 && !w->replicated) (void)mi_shard_range(n_after, c->rank, c->world, &lo, &hi);
    MI_TRY(cpd_load(c, w, before_xyz, m_before, after_xyz + 3 * (size_t)lo, hi - lo));
    w->n_total = n_after;
    const CpdView v = cpd_view(c, w);
    const CpdRules rules = cpd_rules(params, w->m, w->n_total, w->svd_ieee);
    MI_TRY(cpd_init(c, w, v, rules, params->sigma2_init, params->sigma2_mode));
    MI_TRY(cpd_fetch(c, w));
    int batch = params->sync_every;
    if (batch <= 0) batch = cpd_sync_every_estimate(m_before, n_after, w->replicated ? 1 : c->world);
    const bool approximated = params->approximation != MI_CPD_APPROX_NONE;
    if (approximated) batch = 1;                                  // the E-step's shape depends on sigma^2: host-stepped
    // exact P in batches: a host check only peeks (state copy behind the batch, ONE iteration of the next batch behind the copy, the host
    // waits for the copy alone) -- the device does not idle for the ~26 us a drained stream and a fresh enqueue cost (mi_icp_run does the same)
    const bool pipelined = batch > 1 && c->peek_event != nullptr && c->tune.icp_pipeline != 0 && !c->prof.on;
    bool ahead = false;
    while (!w->h_state->done) {
        for (int b = ahead ? 1 : 0; b < batch; b++) MI_TRY(cpd_iteration_enqueue(c, w, v, rules, params));
        if (approximated && c->peek_event != nullptr) {
            // the state copy first, the replay BEHIND it: the host has sigma^2 while the device replays
            MI_TRY(cpd_peek_begin(c, w));
            MI_TRY(cpd_fgt_prelaunch(c, w, v));
            MI_TRY(cpd_peek_wait(c));
        } else if (pipelined) {
            MI_TRY(cpd_peek_begin(c, w));
            MI_TRY(cpd_iteration_enqueue(c, w, v, rules, params));   // (returns at once on the device if the state copied above says "done")
            ahead = true;
            MI_TRY(cpd_peek_wait(c));
        } else
            MI_TRY(cpd_fetch(c, w));
        if (params->verbose) printf("loop_nr %d, error: %f\n", w->h_state->iterations, w->h_state->error);
    }
    // The host checks above only PEEK: behind the state copy that said "done" the stream still holds the iteration enqueued ahead of it (kernels
    // that return at once) or the prelaunched K-centre replay.  Drained here, so that the call's wall time brackets all of its device work
    // (bench.py's timers around this call used to miss that tail) and the workspace is quiet when the caller gets it back.
    MI_HIP(hipStreamSynchronize(c->stream));
    cpd_state_to_outputs(w->h_state, out_sR_t, out_scale, iterations, error);
    w->last_call = c->entered;
    return MI_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// batched CPD: many small exact-P registrations under one set of rules (cpd_batch.hip)
// ---------------------------------------------------------------------------------------------------------------
// Sizes the batched kernel is routed: decided by measurement (DESIGN.md section 4, K-batch CPD): at 64 problems of 2 048 x 2 048 the
// batch beats the loop of single calls, at 4 096 x 4 096 it lost; the kernel is sized to the routed edge
constexpr int CPD_BATCH_ROUTE_MAX = CPD_BATCH_MAX_POINTS;

extern "C" int mi_cpd_batch_route(int m_before, int n_after, const mi_cpd_params* params)
{
    if (!params || m_before < 1 || n_after < 1) return 0;
    if (params->approximation != MI_CPD_APPROX_NONE) return 0;                  // the FGT / hybrid E-steps are host-stepped and cluster whole clouds
    if (params->estep_mode != MI_ESTEP_DEFAULT || params->verbose != 0) return 0;   // the sequential parity sums and the per-iteration print are the single path's
    if (params->sigma2_mode != MI_SIGMA2_EXACT && !(params->sigma2_init > 0.f)) return 0;
    return m_before <= CPD_BATCH_ROUTE_MAX && n_after <= CPD_BATCH_ROUTE_MAX ? 1 : 0;
}

extern "C" int mi_cpd_register_batch(mi_ctx* c, int n_problems, const float* before_xyz, const int* before_range, const float* after_xyz,
                                     const int* after_range, const mi_cpd_params* params, float* out_sR_t, float* out_scale, int* iterations,
                                     float* error, int* stop_reason, mi_cpd_batch_info* info)
{
    if (info) memset(info, 0, sizeof *info);
    if (!c) { set_error("CPD: null context"); return MI_ERR_INVALID_ARG; }       // (code and message of mi_cpd_register)
    if (n_problems < 0) { set_error("mi_cpd_register_batch: n_problems = %d", n_problems); return MI_ERR_INVALID_ARG; }
    if (c->distributed()) { set_error("mi_cpd_register_batch: single-GPU contexts only"); return MI_ERR_STATE; }
    // what mi_cpd_register refuses whatever the sizes
    if (!params) { set_error("mi_cpd_register_batch: null parameters"); return MI_ERR_INVALID_ARG; }
    MI_TRY(cpd_check_params(params, c->world, "mi_cpd_register_batch"));
    if (n_problems == 0) return MI_OK;
    if (!before_xyz || !after_xyz || !before_range || !after_range) { set_error("mi_cpd_register_batch: null cloud or range array"); return MI_ERR_INVALID_ARG; }
    if (!out_sR_t || !iterations || !error || !stop_reason) { set_error("mi_cpd_register_batch: out_sR_t, iterations, error and stop_reason must be non-null"); return MI_ERR_INVALID_ARG; }
    // A context whose single path takes the VALU contraction (MISLAM_CPD_MFMA=0: two roundings per product) computes other bits than the
    // matrix-pipe chain the batched kernel is built on: such a context sends every problem through the single path.
    const bool kernel_follows = c->tune.cpd_mfma != 0;
    std::vector<CpdBatchProblem> table;
    std::vector<int> batched, fallback;
    BatchSpan span;
    long long max_pairs = 0;
    int max_points = 0;
    for (int k = 0; k < n_problems; k++) {
        const long long bo = before_range[2 * k], bm = before_range[2 * k + 1], ao = after_range[2 * k], an = after_range[2 * k + 1];
        if (bo < 0 || ao < 0 || bm < 1 || an < 1 || bo + bm > 0x7fffffffLL || ao + an > 0x7fffffffLL) {
            set_error("mi_cpd_register_batch: problem %d has an invalid range (before %lld + %lld, after %lld + %lld)", k, bo, bm, ao, an);
            return MI_ERR_INVALID_ARG;
        }
        { char who[64]; snprintf(who, sizeof who, "mi_cpd_register_batch: problem %d", k); MI_TRY(cpd_check_fgt_sizes(params, bm, an, who)); }
        if (!kernel_follows || !mi_cpd_batch_route((int)bm, (int)an, params)) { fallback.push_back(k); continue; }
        batched.push_back(k);
        span.add(bo, bm, ao, an);
        CpdBatchProblem p{};
        p.b_off = (int)bo; p.m = (int)bm; p.a_off = (int)ao; p.n = (int)an;
        const CpdChunkPlan plan = cpd_chunk_plan(c->cu_count, p.m, p.n);      // the single path's chunking of these sizes on this device (cpd_load)
        p.k_chunks = plan.k_chunks; p.k_chunk_len = plan.k_chunk_len; p.x_chunks = plan.x_chunks; p.x_chunk_len = plan.x_chunk_len;
        table.push_back(p);
        max_pairs = std::max(max_pairs, bm * an);
        max_points = std::max(max_points, (int)std::max(bm, an));
    }
    MI_ENTER(c);
    c->prob.icp_loaded = false;                               // as cpd_load: no ICP problem stays loaded
    int launches = 0;
    if (!batched.empty()) {
        const int nb = (int)batched.size();
        for (CpdBatchProblem& p : table) { p.b_off -= (int)span.b_lo; p.a_off -= (int)span.a_lo; }
        MI_TRY(c->bat.cpd_problems.reserve((size_t)nb)); MI_TRY(c->bat.cpd_states.reserve((size_t)nb));
        MI_TRY(batch_upload_clouds(c, before_xyz, after_xyz, span));
        MI_HIP(hipMemcpyAsync(c->bat.cpd_problems.p, table.data(), sizeof(CpdBatchProblem) * (size_t)nb, hipMemcpyHostToDevice, c->stream));
        MI_HIP(hipStreamSynchronize(c->stream));         // (the table is pageable host memory of this frame)
        CpdBatchArgs a{};
        a.before = c->bat.before.p; a.after = c->bat.after.p; a.problems = c->bat.cpd_problems.p;
        a.states = c->bat.cpd_states.p; a.running = c->bat.running.p;
        a.n_problems = nb;
        a.max_points = max_points;
        a.iters = cpd_batch_iters(max_pairs);
        a.sigma2_override = params->sigma2_init;
        a.rules = cpd_rules(params, 0, 0, c->tune.svd_ieee);      // (m, n are set per problem in the kernel)
        MI_HIP(cpd_batch_init(a, c->stream));
        MI_TRY(batch_run_until_quiet(c, params->max_iterations > 0, [&] { return cpd_batch_iterate(a, c->stream); }, &launches));
        std::vector<CpdState> states((size_t)nb);
        MI_HIP(hipMemcpyAsync(states.data(), c->bat.cpd_states.p, sizeof(CpdState) * (size_t)nb, hipMemcpyDeviceToHost, c->stream));
        MI_HIP(hipStreamSynchronize(c->stream));
        retire_buffers(c);
        for (int i = 0; i < nb; i++) {
            const int k = batched[(size_t)i];
            cpd_state_to_outputs(&states[(size_t)i], out_sR_t + 16 * (size_t)k, out_scale ? out_scale + k : nullptr, iterations + k, error + k);
            stop_reason[k] = states[(size_t)i].stop_reason;
        }
    }
    for (int k : fallback) {                             // the existing path, one after the other
        const float* b = before_xyz + 3 * (size_t)before_range[2 * k];
        const float* a = after_xyz + 3 * (size_t)after_range[2 * k];
        MI_TRY(mi_cpd_register(c, b, before_range[2 * k + 1], a, after_range[2 * k + 1], params, out_sR_t + 16 * (size_t)k,
                               out_scale ? out_scale + k : nullptr, iterations + k, error + k));
        stop_reason[k] = c->cpd->h_state->stop_reason;   // (the state block the single call's last host check read: the one that said "done")
    }
    if (info) { info->problems_batched = (int)batched.size(); info->problems_fallback = (int)fallback.size(); info->launches = launches; }
    return MI_OK;
}

// How every primitive opens, behind its checks and MI_ENTER: the workspace, unsharded (a primitive runs on single-GPU contexts), both clouds
// loaded and the view over them.  mi_cpd_register has its own opening: it shards.
static int cpd_open_whole(mi_ctx* c, const float* before_xyz, int m, const float* after_xyz, int n, CpdWorkspace** w, CpdView* v)
{
    MI_TRY(cpd_workspace(c, w));
    (*w)->replicated = false;
    (*w)->queries_sharded = false;
    MI_TRY(cpd_load(c, *w, before_xyz, m, after_xyz, n));
    *v = cpd_view(c, *w);
    return MI_OK;
}

extern "C" int mi_cpd_sigma_squared(mi_ctx* c, const float* before_xyz, int m, const float* after_xyz, int n, float* sigma2)
{
    return mi_cpd_sigma_squared_mode(c, before_xyz, m, after_xyz, n, MI_SIGMA2_EXACT, sigma2);
}

extern "C" int mi_cpd_sigma_squared_mode(mi_ctx* c, const float* before_xyz, int m, const float* after_xyz, int n, int sigma2_mode,
                                         float* sigma2)
{
    MI_TRY(cpd_check(c, before_xyz, m, after_xyz, n));
    if (!sigma2) { set_error("mi_cpd_sigma_squared: null output"); return MI_ERR_INVALID_ARG; }
    if (sigma2_mode != MI_SIGMA2_EXACT && sigma2_mode != MI_SIGMA2_CPU_SEQUENTIAL) { set_error("mi_cpd_sigma_squared: bad sigma2_mode %d", sigma2_mode); return MI_ERR_INVALID_ARG; }
    MI_ENTER(c);
    CpdWorkspace* w = nullptr;
    CpdView v{};
    MI_TRY(cpd_open_whole(c, before_xyz, m, after_xyz, n, &w, &v));
    mi_cpd_params p;
    mi_cpd_params_default(&p);
    p.max_iterations = 1;
    MI_TRY(cpd_init(c, w, v, cpd_rules(&p, w->m, w->n_total, w->svd_ieee), 0.f, sigma2_mode));
    MI_TRY(cpd_fetch(c, w));
    *sigma2 = w->h_state->sigma2_init;
    return MI_OK;
}

// The three E-step flavours behind one primitive.  What a flavour does not read stays zero.
enum class EstepKind { Exact, Truncated, Fgt };
struct EstepInputs {
    float constant, sigma2;                                      // Exact, Truncated; sigma2: all three
    float truncate;                                              // Truncated
    float weight, sigma2_init, ratio_of_far_field; int order;    // Fgt
};
static int estep_primitive(mi_ctx* c, const float* y_xyz, int m, const float* x_xyz, int n, EstepKind kind, const EstepInputs& in,
                           float* p1, float* pt1, float* px, float* L)
{
    const float sigma2 = in.sigma2;
    MI_TRY(cpd_check(c, y_xyz, m, x_xyz, n));
    if (!p1 || !pt1 || !px || !L) { set_error("CPD E-step: null output"); return MI_ERR_INVALID_ARG; }
    if (!(sigma2 > 0.f)) { set_error("CPD E-step: sigma2 must be positive"); return MI_ERR_INVALID_ARG; }
    MI_ENTER(c);
    CpdWorkspace* w = nullptr;
    CpdView v{};
    MI_TRY(cpd_open_whole(c, y_xyz, m, x_xyz, n, &w, &v));
    memset(w->h_state, 0, sizeof(CpdState));
    w->h_state->sigma2 = sigma2;
    w->h_state->constant = in.constant;
    w->h_state->scale = 1.f;
    MI_HIP(hipMemcpyAsync(w->d_state.p, w->h_state, sizeof(CpdState), hipMemcpyHostToDevice, c->stream));
    if (kind == EstepKind::Fgt) {
        MI_TRY(cpd_estep_fgt_enqueue(c, w, v, in.weight, sigma2, in.sigma2_init, in.ratio_of_far_field, in.order));
    } else {
        if (kind == EstepKind::Truncated) {
            if (!(in.truncate > 0.f)) { set_error("mi_cpd_estep_truncated: truncate must be positive"); return MI_ERR_INVALID_ARG; }
            v.truncate = 1;
            v.trunc_log = std::log(in.truncate);
        }
        if (kind == EstepKind::Truncated && c->tune.cpd_trunc_cull != 0) MI_TRY(cpd_estep_trunc_enqueue(c, w, v));
        else MI_TRY(cpd_estep_enqueue(c, w, v, MI_ESTEP_DEFAULT));
    }
    w->sums.drop();                      // (a stand-alone E-step: nothing of it is carried into a later M-step call)
    const int nxb = cpd_standalone_sum_blocks(n);
    MI_HIP(cpd_xsums(v, w->part_x.p, nxb, c->stream));
    MI_HIP(hipMemcpyAsync(p1, w->p1.p, sizeof(float) * (size_t)m, hipMemcpyDeviceToHost, c->stream));
    MI_HIP(hipMemcpyAsync(pt1, w->pt1.p, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    MI_HIP(hipMemcpyAsync(px, w->px.p, sizeof(float) * 3 * (size_t)m, hipMemcpyDeviceToHost, c->stream));
    std::vector<double> part((size_t)nxb * CPD_XSUMS);
    MI_HIP(hipMemcpyAsync(part.data(), w->part_x.p, sizeof(double) * part.size(), hipMemcpyDeviceToHost, c->stream));
    MI_HIP(hipStreamSynchronize(c->stream));
    double logsum = 0.0;
    for (int b = 0; b < nxb; b++) logsum += part[(size_t)b * CPD_XSUMS];
    *L = (float)(-logsum) + (float)(3 * n) * logf(sigma2) / 2.0f;     // coherentpointdrift.cpp:215-217 / cpdutils.cpp:69-72
    return MI_OK;
}

extern "C" int mi_cpd_estep(mi_ctx* c, const float* y_xyz, int m, const float* x_xyz, int n, float constant, float sigma2,
                            float* p1, float* pt1, float* px, float* L)
{
    EstepInputs in{};
    in.constant = constant; in.sigma2 = sigma2;
    return estep_primitive(c, y_xyz, m, x_xyz, n, EstepKind::Exact, in, p1, pt1, px, L);
}

extern "C" int mi_cpd_estep_truncated(mi_ctx* c, const float* y_xyz, int m, const float* x_xyz, int n, float constant, float sigma2,
                                      float truncate, float* p1, float* pt1, float* px, float* L)
{
    EstepInputs in{};
    in.constant = constant; in.sigma2 = sigma2; in.truncate = truncate;
    return estep_primitive(c, y_xyz, m, x_xyz, n, EstepKind::Truncated, in, p1, pt1, px, L);
}

extern "C" int mi_cpd_estep_fgt(mi_ctx* c, const float* y_xyz, int m, const float* x_xyz, int n, float weight, float sigma2,
                                float sigma2_init, float ratio_of_far_field, int order_of_truncation,
                                float* p1, float* pt1, float* px, float* L)
{
    if (!(sigma2_init > 0.f)) { set_error("mi_cpd_estep_fgt: sigma2_init must be positive"); return MI_ERR_INVALID_ARG; }
    if (!(weight > 0.f && weight < 1.f)) { set_error("mi_cpd_estep_fgt: weight must lie in (0, 1)"); return MI_ERR_INVALID_ARG; }
    EstepInputs in{};
    in.sigma2 = sigma2; in.weight = weight; in.sigma2_init = sigma2_init; in.ratio_of_far_field = ratio_of_far_field; in.order = order_of_truncation;
    return estep_primitive(c, y_xyz, m, x_xyz, n, EstepKind::Fgt, in, p1, pt1, px, L);
}

extern "C" int mi_cpd_mstep(mi_ctx* c, const float* before_xyz, int m, const float* after_xyz, int n, const float* p1,
                            const float* pt1, const float* px, int const_scale, float out_R9[9], float out_t3[3], float* scale,
                            float* sigma2)
{
    MI_TRY(cpd_check(c, before_xyz, m, after_xyz, n));
    if (!p1 || !pt1 || !px || !out_R9 || !out_t3 || !scale || !sigma2) { set_error("mi_cpd_mstep: null argument"); return MI_ERR_INVALID_ARG; }
    MI_ENTER(c);
    CpdWorkspace* w = nullptr;
    CpdView v{};
    MI_TRY(cpd_open_whole(c, before_xyz, m, after_xyz, n, &w, &v));
    v.xw4 = nullptr;   // no E-step ran: skip the log-likelihood term
    w->sums.drop();
    MI_HIP(hipMemcpyAsync(w->p1.p, p1, sizeof(float) * (size_t)m, hipMemcpyHostToDevice, c->stream));
    MI_HIP(hipMemcpyAsync(w->pt1.p, pt1, sizeof(float) * (size_t)n, hipMemcpyHostToDevice, c->stream));
    MI_HIP(hipMemcpyAsync(w->px.p, px, sizeof(float) * 3 * (size_t)m, hipMemcpyHostToDevice, c->stream));
    memset(w->h_state, 0, sizeof(CpdState));
    w->h_state->scale = *scale;
    w->h_state->sigma2 = *sigma2;
    MI_HIP(hipMemcpyAsync(w->d_state.p, w->h_state, sizeof(CpdState), hipMemcpyHostToDevice, c->stream));
    mi_cpd_params p;
    mi_cpd_params_default(&p);
    p.const_scale = const_scale;
    w->last_estep = -1;
    MI_TRY(cpd_mstep_enqueue(c, w, v, cpd_rules(&p, w->m, w->n_total, w->svd_ieee), 0));
    MI_TRY(cpd_fetch(c, w));
    w->last_call = c->entered;
    memcpy(out_R9, w->h_state->R, sizeof(float) * 9);
    memcpy(out_t3, w->h_state->t, sizeof(float) * 3);
    *scale = w->h_state->scale;
    *sigma2 = w->h_state->sigma2;
    return MI_OK;
}

// Test-only read-back of what the last mi_cpd_register / mi_cpd_mstep left in the workspace (mi_slam.h).  Copies only: no kernel, no state change.
extern "C" int mi_selftest_cpd_last(mi_ctx* c, int m, int n, float* p1, float* pt1, float* px, float* y_xyz, double xs[5], double ks[14],
                                    float R9[9], float t3[3], float* scale, float* sigma2, float* sigma2_init, float* constant, int info[8])
{
    if (!c) { set_error("mi_selftest_cpd_last: null context"); return MI_ERR_INVALID_ARG; }
    CpdWorkspace* w = c->cpd;
    // (any other entry point on the context since then may have reused the moving cloud's buffers: the read-back must be the next call)
    if (!w || w->last_call == 0 || w->last_call != c->entered) { set_error("mi_selftest_cpd_last: the last call on this context was no mi_cpd_register / mi_cpd_mstep"); return MI_ERR_STATE; }
    if (m != w->m || n != w->n) { set_error("mi_selftest_cpd_last: sizes (%d, %d) are not the loaded ones (%d, %d)", m, n, w->m, w->n); return MI_ERR_STATE; }
    MI_ENTER(c);
    w->last_call = c->entered;           // (a read-back may be repeated)
    std::vector<float> soa;
    if (y_xyz) soa.resize(3 * (size_t)m);
    if (p1) MI_HIP(hipMemcpyAsync(p1, w->p1.p, sizeof(float) * (size_t)m, hipMemcpyDeviceToHost, c->stream));
    if (pt1) MI_HIP(hipMemcpyAsync(pt1, w->pt1.p, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    if (px) MI_HIP(hipMemcpyAsync(px, w->px.p, sizeof(float) * 3 * (size_t)m, hipMemcpyDeviceToHost, c->stream));
    if (y_xyz) {
        const float* src[3] = {c->cx.p, c->cy.p, c->cz.p};
        for (int d = 0; d < 3; d++) MI_HIP(hipMemcpyAsync(soa.data() + (size_t)d * m, src[d], sizeof(float) * (size_t)m, hipMemcpyDeviceToHost, c->stream));
    }
    MI_HIP(hipStreamSynchronize(c->stream));
    if (y_xyz)
        for (size_t i = 0; i < (size_t)m; i++)
            for (int d = 0; d < 3; d++) y_xyz[3 * i + d] = soa[(size_t)d * m + i];
    const CpdState* s = w->h_state;      // (as cpd_fetch left it)
    if (xs) memcpy(xs, s->xs, sizeof(double) * 5);
    if (ks) memcpy(ks, s->ks, sizeof(double) * 14);
    if (R9) memcpy(R9, s->R, sizeof(float) * 9);
    if (t3) memcpy(t3, s->t, sizeof(float) * 3);
    if (scale) *scale = s->scale;
    if (sigma2) *sigma2 = s->sigma2;
    if (sigma2_init) *sigma2_init = s->sigma2_init;
    if (constant) *constant = s->constant;
    if (info) {
        info[0] = w->last_estep; info[1] = w->last_fused; info[2] = w->last_rows_x; info[3] = w->last_rows_k;
        info[4] = w->last_reduced; info[5] = s->iterations; info[6] = s->stop_reason; info[7] = 0;
    }
    return MI_OK;
}
