// The ICP driver behind the C ABI, the batched registration and the test-grade ICP primitives.
//
// The ICP driver is the MI355X-native counterpart of CudaICP (source/cuda-slam/icpcuda.cu:8-58): the same loop, but the
// whole iteration -- search, (all-reduce), moments, solve, transform, error, stop rule -- is enqueued on one HIP stream
// without a single host round trip; the host only reads the 256-byte state block back every `sync_every` iterations.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "context.h"

using namespace mislam;

namespace mislam {

// rows of partial sums for the loaded moving cloud (icp_rows.hpp) + the reduced rows
static int reserve_rows(mi_ctx* c)
{
    const size_t rows = (size_t)icp_row_count(c->prob.n_pad) * (ICP_MOMENTS + ICP_ERRSUMS);
    if (rows > c->rows.cap) {
        MI_TRY(c->rows.reserve(rows));
        MI_HIP(hipMemsetAsync(c->rows.p, 0, sizeof(double) * c->rows.cap, c->stream));   // columns a path never writes stay finite
    }
    MI_TRY(c->rows_reduced.reserve((size_t)ICP_REDUCED_ROWS * (ICP_MOMENTS + ICP_ERRSUMS)));
    MI_HIP(hipMemsetAsync(c->rows_reduced.p, 0, sizeof(double) * ICP_REDUCED_ROWS * (ICP_MOMENTS + ICP_ERRSUMS), c->stream));   // (rows past a rank's count: zero)
    MI_TRY(c->sched.order.reserve((size_t)icp_row_count(c->prob.n_pad)));
    MI_TRY(c->sched.far.reserve((size_t)icp_row_count(c->prob.n_pad)));
    MI_TRY(c->sched.lanes.reserve((size_t)icp_row_count(c->prob.n_pad)));
    MI_TRY(c->sched.counters.reserve(ICP_SCHED_CURSORS));
    MI_TRY(c->sched.ticket.reserve(32));                   // (one word in use: a cache line away from the cursors' atomics)
    return MI_OK;
}

static IcpSchedule make_schedule(mi_ctx* c)
{
    IcpSchedule s{};
    s.order = c->sched.order.p; s.far = c->sched.far.p; s.counters = c->sched.counters.p; s.lanes = c->sched.lanes.p;
    s.ticket = c->sched.ticket.p;
    return s;
}

static IcpView make_view(mi_ctx* c)
{
    IcpView v{};
    v.state = c->d_state;
    v.bx = c->bx.p; v.by = c->by.p; v.bz = c->bz.p;
    v.cx = c->cx.p; v.cy = c->cy.p; v.cz = c->cz.p;
    v.tgt4 = c->tgt4.p;
    v.keys = c->keys.p;
    v.n = c->prob.n; v.n_pad = c->prob.n_pad;
    v.shard_lo = c->prob.shard_lo; v.shard_hi = c->prob.shard_hi;
    v.filter_pairs = c->prob.icp.filter_pairs;
    v.max_distance_squared = c->prob.icp.max_distance_squared;
    v.fma = c->prob.icp.dist_mode == MI_DIST_FMA;
    const bool seq = c->prob.icp.sum_mode == MI_SUM_CPU_SEQUENTIAL;
    v.inv_order = seq ? c->sinv.p : nullptr;
    v.resid = seq ? c->resid.p : nullptr;
    return v;
}

static int copy_before_to_current(mi_ctx* c)            // transformedCloud = cloudBefore (basicicp.cpp:30), all n_pad entries
{
    const size_t bytes = sizeof(float) * (size_t)c->prob.n_pad;
    MI_HIP(hipMemcpyAsync(c->cx.p, c->bx.p, bytes, hipMemcpyDeviceToDevice, c->stream));
    MI_HIP(hipMemcpyAsync(c->cy.p, c->by.p, bytes, hipMemcpyDeviceToDevice, c->stream));
    MI_HIP(hipMemcpyAsync(c->cz.p, c->bz.p, bytes, hipMemcpyDeviceToDevice, c->stream));
    return MI_OK;
}

static void state_identity(IcpState* s)
{
    memset(s, 0, sizeof *s);
    s->R[0] = s->R[4] = s->R[8] = 1.f;
    s->prevR[0] = s->prevR[4] = s->prevR[8] = 1.f;
    s->error = 1e5f;                 // "*error = 1e5"  basicicp.cpp:26
    s->prev_error = 3.402823466e38f; // numeric_limits<float>::max()  icpcuda.cu:10
}

}  // namespace mislam

// ---------------------------------------------------------------------------------------------------------------
// ICP
// ---------------------------------------------------------------------------------------------------------------
extern "C" void mi_icp_params_default(mi_icp_params* p)
{
    if (!p) return;
    memset(p, 0, sizeof *p);
    p->eps = 1e-3f;
    p->max_iterations = -1;
    p->max_distance_squared = 1000.f;
    p->dist_mode = MI_DIST_CPU_ROUNDING;
    p->compose_mode = MI_COMPOSE_CPU_ADDITIVE;
    p->filter_pairs = 1;
    p->abort_on_increase = 0;
    p->sync_every = 0;
    p->verbose = 0;
}

extern "C" void mi_icp_params_cuda_slam(mi_icp_params* p)
{
    if (!p) return;
    mi_icp_params_default(p);
    p->dist_mode = MI_DIST_FMA;
    p->compose_mode = MI_COMPOSE_EXACT;
    p->filter_pairs = 0;
    p->abort_on_increase = 1;
}

static int icp_check_params(const mi_icp_params* p)
{
    if (!p) { set_error("ICP: null params"); return MI_ERR_INVALID_ARG; }
    if (p->dist_mode != MI_DIST_CPU_ROUNDING && p->dist_mode != MI_DIST_FMA) { set_error("ICP: bad dist_mode %d", p->dist_mode); return MI_ERR_INVALID_ARG; }
    if (p->compose_mode != MI_COMPOSE_CPU_ADDITIVE && p->compose_mode != MI_COMPOSE_EXACT) { set_error("ICP: bad compose_mode %d", p->compose_mode); return MI_ERR_INVALID_ARG; }
    if (p->max_iterations < -1) { set_error("ICP: max_iterations %d (use -1 for unbounded)", p->max_iterations); return MI_ERR_INVALID_ARG; }
    if (p->nn_mode != MI_NN_AUTO && p->nn_mode != MI_NN_BRUTEFORCE && p->nn_mode != MI_NN_TREE && p->nn_mode != MI_NN_GRID) { set_error("ICP: bad nn_mode %d", p->nn_mode); return MI_ERR_INVALID_ARG; }
    if (p->shard_mode != MI_SHARD_AUTO && p->shard_mode != MI_SHARD_TARGET && p->shard_mode != MI_SHARD_SOURCE) { set_error("ICP: bad shard_mode %d", p->shard_mode); return MI_ERR_INVALID_ARG; }
    if (p->sum_mode != MI_SUM_EXACT && p->sum_mode != MI_SUM_CPU_SEQUENTIAL) { set_error("ICP: bad sum_mode %d", p->sum_mode); return MI_ERR_INVALID_ARG; }
    return MI_OK;
}

extern "C" int mi_icp_reset(mi_ctx* c)
{
    if (!c || !c->prob.icp_loaded) { set_error("mi_icp_reset: no problem loaded"); return MI_ERR_STATE; }
    MI_ENTER(c);
    state_identity(c->h_state);
    c->prob.enqueued_passes = 0;
    if (c->prob.icp.max_iterations == 0) {   // "while (iterations < maxIterations)" never enters
        c->h_state->done = 1;
        c->h_state->stop_reason = MI_STOP_MAX_ITERATIONS;
    }
    MI_HIP(hipMemcpyAsync(c->d_state, c->h_state, sizeof(IcpState), hipMemcpyHostToDevice, c->stream));
    MI_TRY(copy_before_to_current(c));
    MI_HIP(fill_keys(c->keys.p, c->prob.n, c->stream));
    if (c->prob.fused) {
        MI_TRY(c->grid.match_slot.reserve((size_t)c->prob.n_pad));
        MI_HIP(hipMemsetAsync(c->grid.match_slot.p, 0xff, sizeof(unsigned int) * (size_t)c->prob.n, c->stream));   // ~0u: no match yet
    }
    MI_HIP(icp_schedule_reset(make_schedule(c), icp_row_count(c->prob.n), c->stream));
    MI_HIP(hipStreamSynchronize(c->stream));
    retire_buffers(c);
    return MI_OK;
}

extern "C" int mi_icp_load(mi_ctx* c, const float* before_xyz, int n_before, const float* after_xyz, int n_after,
                           const mi_icp_params* params)
{
    if (!c) { set_error("mi_icp_load: null context"); return MI_ERR_INVALID_ARG; }
    if (!before_xyz || !after_xyz || n_before <= 0 || n_after <= 0) { set_error("mi_icp_load: empty or null cloud (n_before=%d, n_after=%d)", n_before, n_after); return MI_ERR_INVALID_ARG; }
    if (n_after < c->world || n_before < c->world) { set_error("mi_icp_load: fewer points (%d, %d) than ranks (%d)", n_before, n_after, c->world); return MI_ERR_INVALID_ARG; }
    MI_TRY(icp_check_params(params));
    if (params->sum_mode == MI_SUM_CPU_SEQUENTIAL && c->distributed()) { set_error("mi_icp_load: MI_SUM_CPU_SEQUENTIAL needs a single-GPU context (the running sums follow one global point order)"); return MI_ERR_INVALID_ARG; }
    MI_ENTER(c);
    StageClock clock(c, c->prob.load_ms);      // mi_icp_load_times: time since the last mark -> `stage`, its device allocations -> stage 0
    c->prob.icp_loaded = false;
    c->prob.icp = *params;
    // what the ranks split (mi_slam.h MI_SHARD_*): decided from GLOBAL sizes, so every rank decides alike
    c->prob.source_sharded = false;
    if (c->distributed()) {   // (a one-rank communicator takes the same path: that is what the single-GPU box can test)
        const int per_rank = n_after / c->world;
        const bool indexed = resolve_nn_mode(c, params->nn_mode, params->shard_mode == MI_SHARD_TARGET ? per_rank : n_after) != MI_NN_BRUTEFORCE;
        c->prob.source_sharded = params->shard_mode == MI_SHARD_SOURCE || (params->shard_mode == MI_SHARD_AUTO && indexed);
    }
    // Source sharding.  A rank's moving points should be (a) spatially DENSE wave by wave -- a wave's 64 points walk the box
    // hierarchy together, and sparse waves walk longer -- and (b) the same mix of easy and hard regions on every rank.  So every
    // rank orders the WHOLE moving cloud along the Hilbert curve (1 ms) and keeps the 64-point chunks rank, rank + W, rank + 2W ...
    // of that order.  (Clouds too small for a few chunks per rank are cut into contiguous slices of the caller's order instead.)
    const int n_all = n_before;
    c->prob.n_global = n_all;
    const bool deal_chunks = c->prob.source_sharded && n_all >= 4 * ICP_CHUNK_POINTS * c->world;
    if (c->prob.source_sharded && !deal_chunks) {
        int slo = 0, shi = 0;
        (void)mi_shard_range(n_before, c->rank, c->world, &slo, &shi);
        before_xyz += 3 * (size_t)slo;
        n_before = shi - slo;
    }
    if (deal_chunks) MI_TRY(mi_source_share(n_all, c->rank, c->world, &n_before));
    c->prob.n = n_before;
    c->prob.n_pad = round_up(n_before, NN_SRC_PAD);
    const size_t np = (size_t)c->prob.n_pad;
    const int all_pad = round_up(n_all, NN_SRC_PAD);
    MI_TRY(reserve_moving(c, np, deal_chunks ? (size_t)all_pad : np));      // (cx.. hold the whole cloud while it is dealt out)
    MI_TRY(reserve_rows(c));
    MI_TRY(clock.mark(0));
    if (deal_chunks) {
        MI_TRY(c->ax.reserve((size_t)all_pad)); MI_TRY(c->ay.reserve((size_t)all_pad)); MI_TRY(c->az.reserve((size_t)all_pad));
        MI_TRY(upload_soa(c, before_xyz, n_all, all_pad, c->cx.p, c->cy.p, c->cz.p, nullptr));
        MI_TRY(clock.mark(1));
        MI_TRY(sort_sources(c, c->cx.p, c->cy.p, c->cz.p, n_all, all_pad, c->ax.p, c->ay.p, c->az.p));
        MI_HIP(deal_chunks_soa(c->ax.p, c->ay.p, c->az.p, n_all, c->rank, c->world, c->prob.n, c->prob.n_pad, c->bx.p, c->by.p, c->bz.p, c->stream));
        MI_TRY(clock.mark(2));
    } else {
        // moving cloud: upload in the caller's order (cx.. as scratch), keep it Hilbert-sorted in bx..
        MI_TRY(upload_soa(c, before_xyz, n_before, c->prob.n_pad, c->cx.p, c->cy.p, c->cz.p, nullptr));
        MI_TRY(clock.mark(1));
        MI_TRY(sort_sources(c, c->cx.p, c->cy.p, c->cz.p, n_before, c->prob.n_pad, c->bx.p, c->by.p, c->bz.p));
        MI_TRY(clock.mark(2));
    }
    if (params->sum_mode == MI_SUM_CPU_SEQUENTIAL) {   // the sequential sums run in the CALLER's point order
        MI_TRY(c->sinv.reserve((size_t)n_before));
        MI_TRY(c->resid.reserve(np));
        MI_HIP(invert_order(c->sorder.p, n_before, c->sinv.p, c->stream));
    }
    MI_TRY(clock.mark(2));
    // The FIXED cloud's share of the load -- upload, box hierarchy, cell grid -- depends on nothing the moving cloud's does, so it runs
    // on its own lanes (round 4): the upload and the hierarchy on `aux`, the grid (behind the upload) on `aux2`, their own scratch sets,
    // while `stream` is still ordering the moving cloud.  The host only copies into the pinned ring and enqueues; its one wait -- the grid's
    // bounding box -- is a wait for the fixed cloud's upload, which it would have sat out anyway.  `stream` then waits for both lanes.
    // (With profiling on, everything stays on `stream`, stage by stage: mi_icp_load_times drains it at every mark.)
    const bool lanes = !c->prof.on && c->aux != nullptr && c->aux2 != nullptr;
    const int m_local_pre = [&] { int lo = 0, hi = n_after; if (!c->prob.source_sharded) (void)mi_shard_range(n_after, c->rank, c->world, &lo, &hi); return hi - lo; }();
    // The grid search carries the whole O(N) part of the iteration (nn_grid.hip) unless a stand-alone step has to come between
    // the search and the sums: the key all-reduce of a sharded fixed cloud, or cpu-slam's sequential running sums.
    const int mode = resolve_nn_mode(c, params->nn_mode, m_local_pre);
    // Every way out of this function joins the lanes into `stream`: an early return between here and the join below -- the
    // hierarchy refusing an over-tall cloud, a failed reserve -- used to leave work on aux / aux2 that `stream`, the only stream the next call's
    // buffer retirement and ~CtxScope look at, knew nothing about.
    struct LaneJoin {
        mi_ctx* c; bool on; bool joined = false;
        ~LaneJoin()
        {
            if (!on || joined) return;
            if (hipEventRecord(c->aux_event[1], c->aux) == hipSuccess) (void)hipStreamWaitEvent(c->stream, c->aux_event[1], 0);
            if (hipEventRecord(c->aux_event[2], c->aux2) == hipSuccess) (void)hipStreamWaitEvent(c->stream, c->aux_event[2], 0);
        }
    } lane_join{c, lanes};
    {
        LaneScope ls(c, lanes ? c->aux : nullptr, lanes ? 1 : 0);
        MI_TRY(upload_target_shard(c, after_xyz, n_after, c->prob.source_sharded));
        if (lanes) MI_HIP(hipEventRecord(c->aux_event[0], c->aux));           // the fixed cloud is on the device
    }
    MI_TRY(clock.mark(3));
    const int m_local = c->prob.shard_hi - c->prob.shard_lo;
    c->prob.fused = mode == MI_NN_GRID && (!c->distributed() || c->prob.source_sharded) && params->sum_mode == MI_SUM_EXACT;
    if (mode != MI_NN_BRUTEFORCE) {          // build the indexes now, not inside the first timed iteration
        {
            LaneScope ls(c, lanes ? c->aux : nullptr, lanes ? 1 : 0);
            MI_TRY(ensure_tree(c, m_local, c->prob.shard_lo));
        }
        MI_TRY(clock.mark(4));
        if (mode == MI_NN_GRID) {
            if (lanes) MI_HIP(hipStreamWaitEvent(c->aux2, c->aux_event[0], 0));
            LaneScope ls(c, lanes ? c->aux2 : nullptr, 0);                    // (the grid build has its own scratch; lane 0's sort scratch is not touched)
            MI_TRY(ensure_grid(c, m_local, c->prob.shard_lo));
        }
        MI_TRY(clock.mark(5));
    }
    if (lanes) {                             // everything after the load runs on `stream`: it waits for both lanes here, once
        MI_HIP(hipEventRecord(c->aux_event[1], c->aux));
        MI_HIP(hipEventRecord(c->aux_event[2], c->aux2));
        MI_HIP(hipStreamWaitEvent(c->stream, c->aux_event[1], 0));
        MI_HIP(hipStreamWaitEvent(c->stream, c->aux_event[2], 0));
        lane_join.joined = true;
    }
    c->prob.icp_loaded = true;
    MI_TRY(mi_icp_reset(c));
    MI_TRY(clock.mark(6));
    clock.finish();
    return MI_OK;
}

extern "C" int mi_icp_load_times(mi_ctx* c, double out_ms[MI_LOAD_STAGES]) { return stage_times("mi_icp_load_times", c ? c->prob.load_ms : nullptr, out_ms); }

// The one place an IcpRules is filled: the loaded problem's, the batch call's, mi_kabsch's (svd_ieee: the context's MISLAM_SVD_IEEE switch)
static IcpRules icp_rules(const mi_icp_params& p, int m_total, int svd_ieee)
{
    IcpRules rules{};
    rules.eps = p.eps;
    rules.max_iterations = p.max_iterations;
    rules.filter_pairs = p.filter_pairs;
    rules.abort_on_increase = p.abort_on_increase;
    rules.m_total = m_total;
    rules.seq_sums = p.sum_mode == MI_SUM_CPU_SEQUENTIAL;
    rules.svd_ieee = svd_ieee;
    return rules;
}
static IcpRules icp_rules(const mi_ctx* c) { return icp_rules(c->prob.icp, c->prob.m_total, c->tune.svd_ieee); }

// The error sums of the last enqueued iteration have not been turned into its stop rule yet (they normally ride with the next
// iteration's moments).  Called when the host stops enqueuing and wants the state.
static int icp_flush_pending(mi_ctx* c)
{
    const IcpView v = make_view(c);
    const int nrows = icp_row_count(c->prob.n);
    const int reduced = icp_reduced_count(nrows);
    // fused path: nobody has evaluated the last applied transform yet -- the next search would have
    if (c->prob.fused) { ProfScope ps(c, MI_KERNEL_TRANSFORM); MI_HIP(icp_transform_error_rows(v, c->rows.p, 0, c->stream)); }
    ProfScope ps(c, MI_KERNEL_FINALIZE);
    MI_HIP(icp_rows_reduce(c->rows.p, nrows, c->rows_reduced.p, c->stream));
    if (c->distributed()) {
        MI_HIP(icp_rows_to_state(c->d_state, c->rows_reduced.p, reduced, 2, c->stream));
        MI_TRY(allreduce_sum_f64(c, c->d_state->err, ICP_ERRSUMS));
        MI_HIP(icp_finalize_pending(c->d_state, nullptr, 0, icp_rules(c), c->stream));
    } else {
        MI_HIP(icp_finalize_pending(c->d_state, c->rows_reduced.p, reduced, icp_rules(c), c->stream));
    }
    return MI_OK;
}

// One loop body of basicicp.cpp:32-57 / icpcuda.cu:31-54, enqueued without host synchronisation.  Two launches on the
// default path: fused search (transform, previous error, search, moments) -> rows reduce whose last workgroup solves (previous
// stop rule, Kabsch, compose).
static int icp_enqueue_iteration(mi_ctx* c)
{
    const IcpView v = make_view(c);
    const int m_local = c->prob.shard_hi - c->prob.shard_lo;
    const IcpRules rules = icp_rules(c);
    const int nrows = icp_row_count(c->prob.n);
    const int reduced = icp_reduced_count(nrows);
    const int seq = c->prob.icp.sum_mode == MI_SUM_CPU_SEQUENTIAL;
    const int parity = c->prob.enqueued_passes & 1;      // which pair of the work order's cursors this step deals on (IcpSchedule)
    if (c->prob.fused) {
        GridSearchArgs a = grid_search_args(c, c->prob.n);
        a.state = c->d_state;
        a.bx = c->bx.p; a.by = c->by.p; a.bz = c->bz.p;
        a.match_slot = c->grid.match_slot.p; a.shard_lo = c->prob.shard_lo; a.shard_hi = c->prob.shard_hi;
        a.filter_pairs = c->prob.icp.filter_pairs; a.max_distance_squared = c->prob.icp.max_distance_squared;
        a.rows = c->rows.p;
        a.order = c->sched.order.p; a.far = c->sched.far.p; a.far_lanes = c->sched.lanes.p;
        // (the host's own count of the iterations it has enqueued since the load / reset: the device's `passes` as long as the registration runs)
        a.extend_reach = c->prob.enqueued_passes < GRID_COLD_PASSES ? 1 : 0;
        a.extend_reach_next = c->prob.enqueued_passes + 1 < GRID_COLD_PASSES ? 1 : 0;
        a.split_walks = c->tune.grid_split_walks < 0 ? (c->prob.n <= GRID_HELPER_FULL_MAX_POINTS ? 1 : (c->prob.n <= GRID_HELPER_MAX_POINTS ? 2 : 0)) : c->tune.grid_split_walks;
        hipEvent_t e0 = nullptr, e1 = nullptr;           // timed, if at all, by events attached to the launch itself (nn_grid_query)
        MI_TRY(c->prof.span(MI_KERNEL_NN, &e0, &e1));
        MI_HIP(nn_grid_query(c->grid.view, c->tree.view, a, v.fma, c->stream, e0, e1));
        c->prob.enqueued_passes += 1;
    } else {
        // K1 (+ C1), K2
        MI_TRY(launch_nn(c, c->cx.p, c->cy.p, c->cz.p, c->prob.n, m_local, c->prob.shard_lo, v.fma, &c->d_state->done, c->prob.icp.nn_mode));
        if (!c->prob.source_sharded) MI_TRY(allreduce_keys(c, c->prob.n));   // source-sharded ranks hold disjoint moving points: nothing to merge
        { ProfScope ps(c, MI_KERNEL_MOMENTS); MI_HIP(icp_moments_rows(v, c->rows.p, c->stream)); }
        if (seq) { ProfScope ps(c, MI_KERNEL_MOMENTS); MI_HIP(icp_seq_centroids(v, c->stream)); }
    }
    {   // K3 (+ K6 of the previous iteration)
        const IcpSchedule sched = make_schedule(c);
        int* cursors = c->prob.fused ? sched.counters : nullptr;
        if (c->distributed()) {
            // ONE all-reduce per iteration: this iteration's 16 moments and the previous iteration's 2 error sums ride together -- as
            // the REDUCED ROWS themselves (64 x 18 doubles, the rows past this rank's own count written as zeros EVERY iteration -- the
            // collective is in place, and a rank with fewer rows than its neighbour would otherwise re-send the neighbour's sums: every
            // rank sends the same length whatever its share), so that the solve kernel adds them up exactly as on one GPU and no kernel sits between
            // the reduction and the collective (a 9 KB all-reduce is as latency-bound as a 144-byte one)
            (void)reduced;
            { ProfScope ps(c, MI_KERNEL_SOLVE); MI_HIP(icp_rows_reduce(c->rows.p, nrows, c->rows_reduced.p, c->stream, c->prob.fused ? &sched : nullptr, true, parity)); }
            { ProfScope ps(c, MI_KERNEL_ALLREDUCE); MI_TRY(allreduce_sum_f64(c, c->rows_reduced.p, ICP_REDUCED_ROWS * (ICP_MOMENTS + ICP_ERRSUMS))); }
            ProfScope ps(c, MI_KERNEL_SOLVE);
            MI_HIP(icp_solve_deferred(c->d_state, c->rows_reduced.p, ICP_REDUCED_ROWS, c->prob.icp.compose_mode, rules, 1, c->stream, cursors));
        } else if (nrows <= ICP_FUSED_SOLVE_MAX_ROWS && c->tune.icp_fused_solve != 0) {
            // small clouds: one launch of one workgroup for both (and no work order: every wave of such a search is resident from the start)
            ProfScope ps(c, MI_KERNEL_SOLVE);
            MI_HIP(icp_reduce_solve(c->d_state, c->rows.p, nrows, c->prob.icp.compose_mode, rules, 1, c->stream));
        } else if (c->tune.icp_ticket_solve != 0 && !seq) {
            // larger clouds: still one launch -- the summing workgroup that arrives last solves (icp_rows_reduce_solve_kernel)
            ProfScope ps(c, MI_KERNEL_SOLVE);
            MI_HIP(icp_rows_reduce_solve(c->d_state, c->rows.p, nrows, c->rows_reduced.p, c->prob.fused ? &sched : nullptr, parity, sched.ticket,
                                         c->prob.icp.compose_mode, rules, 1, c->stream));
        } else {
            ProfScope ps(c, MI_KERNEL_SOLVE);
            MI_HIP(icp_rows_reduce(c->rows.p, nrows, c->rows_reduced.p, c->stream, c->prob.fused ? &sched : nullptr, false, parity));
            MI_HIP(icp_solve_deferred(c->d_state, c->rows_reduced.p, reduced, c->prob.icp.compose_mode, rules, 1, c->stream, cursors));
        }
    }
    if (!c->prob.fused) {
        // K4+K5: its error sums wait in the rows for the next solve (or the flush)
        { ProfScope ps(c, MI_KERNEL_TRANSFORM); MI_HIP(icp_transform_error_rows(v, c->rows.p, 2, c->stream)); }
        if (seq) { ProfScope ps(c, MI_KERNEL_TRANSFORM); MI_HIP(icp_seq_error(v, c->stream)); }
    }
    return MI_OK;
}

static int icp_fetch_state(mi_ctx* c)
{
    { StallProbe sp("fetch_state: enqueue copy"); MI_HIP(hipMemcpyAsync(c->h_state, c->d_state, sizeof(IcpState), hipMemcpyDeviceToHost, c->stream)); }
    { StallProbe sp("fetch_state: stream synchronize"); MI_HIP(hipStreamSynchronize(c->stream)); }
    { StallProbe sp("fetch_state: retire buffers"); retire_buffers(c); }
    return MI_OK;
}

extern "C" int mi_icp_auto_batch(long long n_moving_total, long long m_fixed_total, int world, int source_sharded, int every_pair_search)
{
    if (world < 1) world = 1;
    const double n_rank = (double)n_moving_total / world, m_rank = (double)m_fixed_total / world;
    const double est_s = every_pair_search ? (source_sharded ? n_rank * (double)m_fixed_total : (double)n_moving_total * m_rank) / 7e12
                                           : 2e-5 + 5e-11 * (source_sharded ? n_rank : (double)n_moving_total);
    return est_s >= 5e-3 ? 1 : (est_s >= 2e-4 ? 4 : (est_s >= 1e-4 ? 8 : 16));
}

extern "C" int mi_icp_run(mi_ctx* c, int max_new_iterations, int* iterations_done)
{
    if (!c || !c->prob.icp_loaded) { set_error("mi_icp_run: no problem loaded"); return MI_ERR_STATE; }
    MI_ENTER(c);
    MI_TRY(icp_fetch_state(c));
    const int passes_before = c->h_state->passes;
    int batch = c->prob.icp.sync_every;
    if (batch <= 0) {
        // auto: a long iteration dwarfs a host round trip (check after each one); short ones are launch-bound (batch them).
        // Estimated from the measured rates: every-pair ~7e12 pairs/s, indexed searches ~5e-11 s per moving point + launches.
        // From GLOBAL sizes only: every batch ends in a collective, so all ranks must pick the same batch (a rank's own share
        // of the dealt moving cloud differs from its neighbours' by up to 64 points).
        const bool brute = resolve_nn_mode(c, c->prob.icp.nn_mode, c->prob.source_sharded ? c->prob.m_total : c->prob.m_total / c->world) == MI_NN_BRUTEFORCE;
        batch = mi_icp_auto_batch(c->prob.n_global, c->prob.m_total, c->world, c->prob.source_sharded ? 1 : 0, brute ? 1 : 0);
    }
    if (c->prob.icp.verbose) batch = 1;       // one "loop_nr" line per iteration, like basicicp.cpp:50 / icpcuda.cu:39
    int enqueued = 0;
    // Batches of more than one iteration are PIPELINED (round 4): an intermediate host check used to settle the pending iteration (two
    // launches over the moving cloud, ~23 us at 1e6 points), copy the state and drain the stream -- ~50 us in which the device waits for the
    // host to read one flag and enqueue the next batch.  Now a check only PEEKS: the state block is copied behind the batch, ONE iteration
    // of the next batch goes onto the stream behind the copy, and the host waits for the copy alone; the device is never idle, and the
    // deferred stop rule makes the peek sound (a stop shows up one iteration late and that iteration applies nothing -- exactly as inside
    // a batch; an iteration enqueued behind a stop returns at once).  The pending iteration is settled once, when the loop ends.
    const bool pipelined = batch > 1 && !c->prof.on && g_stall_ms <= 0 && c->peek_event != nullptr && c->tune.icp_pipeline != 0;
    bool ahead = false;                  // one iteration of the next batch is on the stream already
    // a run capped at max_iterations is not enqueued past the cap (the device would turn the surplus into launches that return at once:
    // 14 of them behind a 50-iteration run in batches of 16); `ahead`: the iteration already enqueued counts towards this batch
    const auto batch_len = [&](int ahead_count) {
        const int todo = max_new_iterations >= 0 ? std::min(batch, max_new_iterations - enqueued + ahead_count) : batch;
        return c->prob.icp.max_iterations >= 0 ? std::max(1, std::min(todo, c->prob.icp.max_iterations - c->h_state->iterations)) : todo;
    };
    while (pipelined && !c->h_state->done && (max_new_iterations < 0 || enqueued < max_new_iterations)) {
        const int todo = batch_len(ahead ? 1 : 0);
        for (int b = ahead ? 1 : 0; b < todo; b++) { MI_TRY(icp_enqueue_iteration(c)); enqueued++; }
        const bool last = (max_new_iterations >= 0 && enqueued >= max_new_iterations) ||
                          (c->prob.icp.max_iterations >= 0 && c->h_state->iterations + todo >= c->prob.icp.max_iterations);
        if (last) { ahead = false; break; }                           // (the budget is spent: nothing to decide, settle below)
        MI_HIP(hipMemcpyAsync(c->h_state, c->d_state, sizeof(IcpState), hipMemcpyDeviceToHost, c->stream));
        MI_HIP(hipEventRecord(c->peek_event, c->stream));
        MI_TRY(icp_enqueue_iteration(c));                             // the next batch's first iteration, behind the copy
        enqueued++;
        ahead = true;
        MI_HIP(hipEventSynchronize(c->peek_event));
    }
    if (pipelined) {
        MI_TRY(icp_flush_pending(c));
        MI_TRY(icp_fetch_state(c));
    }
    while (!pipelined && !c->h_state->done && (max_new_iterations < 0 || enqueued < max_new_iterations)) {
        const int todo = batch_len(0);
        hipEvent_t dev_e0 = nullptr, dev_e1 = nullptr;
        if (g_stall_ms > 0) { (void)hipEventCreate(&dev_e0); (void)hipEventCreate(&dev_e1); (void)hipEventRecord(dev_e0, c->stream); }
        { StallProbe sp("run: enqueue batch"); for (int b = 0; b < todo; b++) MI_TRY(icp_enqueue_iteration(c)); }
        { StallProbe sp("run: enqueue flush"); MI_TRY(icp_flush_pending(c)); }
        if (dev_e1) (void)hipEventRecord(dev_e1, c->stream);
        enqueued += todo;
        const int shown = c->h_state->passes;
        MI_TRY(icp_fetch_state(c));
        if (dev_e1) {
            float dev_ms = 0.f;
            (void)hipEventElapsedTime(&dev_ms, dev_e0, dev_e1);
            if (dev_ms > g_stall_ms) fprintf(stderr, "mislam stall: the batch's %d iterations took %.2f ms ON THE DEVICE (events)\n", todo, dev_ms);
            (void)hipEventDestroy(dev_e0); (void)hipEventDestroy(dev_e1);
        }
        if (c->prob.icp.verbose && c->rank == 0 && c->h_state->passes > shown)
            printf("loop_nr %d, error: %f, correspondencesSize: %d\n", c->h_state->passes - 1, c->h_state->error, c->h_state->pairs);
    }
    if (iterations_done) *iterations_done = c->h_state->passes - passes_before;
    return MI_OK;
}

static void state_to_outputs(const IcpState* s, float* out_T, int* iterations, float* error, int* stop_reason)     // (any output may be null)
{
    if (out_T) {
        // column-major 4x4, t in column 3 (ConvertToTransformationMatrix, common.cpp:353-358)
        for (int col = 0; col < 3; col++) {
            for (int row = 0; row < 3; row++) out_T[4 * col + row] = s->R[3 * col + row];
            out_T[4 * col + 3] = 0.f;
        }
        out_T[12] = s->t[0]; out_T[13] = s->t[1]; out_T[14] = s->t[2]; out_T[15] = 1.f;
    }
    if (iterations) *iterations = s->iterations;
    if (error) *error = s->error;
    if (stop_reason) *stop_reason = s->done ? s->stop_reason : MI_STOP_RUNNING;
}

extern "C" int mi_icp_result(mi_ctx* c, float out_T[16], int* iterations, float* error, int* stop_reason)
{
    if (!c || !c->prob.icp_loaded) { set_error("mi_icp_result: no problem loaded"); return MI_ERR_STATE; }
    MI_ENTER(c);
    MI_TRY(icp_fetch_state(c));
    state_to_outputs(c->h_state, out_T, iterations, error, stop_reason);
    return MI_OK;
}

// Test hook: what a step leaves behind besides the result -- the work order dealt for the next search with its flags and cursors, the ticket of
// icp_rows_reduce_solve and the sums the last solve read (state->mom, state->err).
extern "C" int mi_selftest_icp_schedule(mi_ctx* c, int cap_rows, int* order, unsigned char* far, int* rows, int cursors[4], int* ticket, double sums[18])
{
    if (!c || !c->prob.icp_loaded) { set_error("mi_selftest_icp_schedule: no problem loaded"); return MI_ERR_STATE; }
    if (!rows || !cursors || !ticket || !sums || cap_rows < 0 || (cap_rows > 0 && (!order || !far))) { set_error("mi_selftest_icp_schedule: bad argument"); return MI_ERR_INVALID_ARG; }
    MI_ENTER(c);
    static_assert(ICP_SCHED_CURSORS == 4 && ICP_MOMENTS + ICP_ERRSUMS == 18, "the sizes mi_slam.h states");
    const int nrows = icp_row_count(c->prob.n);
    *rows = nrows;
    const size_t take = (size_t)std::min(cap_rows, nrows);
    MI_TRY(icp_fetch_state(c));
    if (take > 0) {
        MI_HIP(hipMemcpyAsync(order, c->sched.order.p, sizeof(int) * take, hipMemcpyDeviceToHost, c->stream));
        MI_HIP(hipMemcpyAsync(far, c->sched.far.p, take, hipMemcpyDeviceToHost, c->stream));
    }
    MI_HIP(hipMemcpyAsync(cursors, c->sched.counters.p, sizeof(int) * ICP_SCHED_CURSORS, hipMemcpyDeviceToHost, c->stream));
    MI_HIP(hipMemcpyAsync(ticket, c->sched.ticket.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    MI_HIP(hipStreamSynchronize(c->stream));
    for (int i = 0; i < ICP_MOMENTS; i++) sums[i] = c->h_state->mom[i];
    for (int i = 0; i < ICP_ERRSUMS; i++) sums[ICP_MOMENTS + i] = c->h_state->err[i];
    return MI_OK;
}

extern "C" int mi_icp_register(mi_ctx* c, const float* before_xyz, int n_before, const float* after_xyz, int n_after,
                               const mi_icp_params* params, float out_T[16], int* iterations, float* error)
{
    if (!iterations || !error || !out_T) { set_error("mi_icp_register: out_T, iterations and error must be non-null"); return MI_ERR_INVALID_ARG; }
    MI_TRY(mi_icp_load(c, before_xyz, n_before, after_xyz, n_after, params));
    MI_TRY(mi_icp_run(c, -1, nullptr));
    return mi_icp_result(c, out_T, iterations, error, nullptr);
}

// ---------------------------------------------------------------------------------------------------------------
// batched ICP: many small registrations under one set of rules (icp_batch.hip)
// ---------------------------------------------------------------------------------------------------------------
extern "C" int mi_icp_batch_route(int n_before, int n_after, const mi_icp_params* params)
{
    if (!params || n_before < 1 || n_after < 1) return 0;
    if (params->sum_mode != MI_SUM_EXACT || params->verbose != 0) return 0;     // the sequential sums and the per-iteration print are the single path's
    return n_before <= ICP_BATCH_MAX_MOVING && n_after <= ICP_BATCH_MAX_FIXED ? 1 : 0;
}

extern "C" int mi_icp_register_batch(mi_ctx* c, int n_problems, const float* before_xyz, const int* before_range, const float* after_xyz,
                                     const int* after_range, const mi_icp_params* params, float* out_T, int* iterations, float* error,
                                     int* stop_reason, mi_icp_batch_info* info)
{
    if (info) memset(info, 0, sizeof *info);
    if (!c) { set_error("mi_icp_register_batch: null context"); return MI_ERR_INVALID_ARG; }
    if (n_problems < 0) { set_error("mi_icp_register_batch: n_problems = %d", n_problems); return MI_ERR_INVALID_ARG; }
    if (c->distributed()) { set_error("mi_icp_register_batch: single-GPU contexts only"); return MI_ERR_STATE; }
    MI_TRY(icp_check_params(params));
    if (n_problems == 0) return MI_OK;
    if (!before_xyz || !after_xyz || !before_range || !after_range) { set_error("mi_icp_register_batch: null cloud or range array"); return MI_ERR_INVALID_ARG; }
    if (!out_T || !iterations || !error || !stop_reason) { set_error("mi_icp_register_batch: out_T, iterations, error and stop_reason must be non-null"); return MI_ERR_INVALID_ARG; }
    // the table of the problems the kernel carries; offsets relative to the first point any of them uses
    std::vector<IcpBatchProblem> table;
    std::vector<int> batched, fallback;
    BatchSpan span;
    long long slots = 0, max_pairs = 0;
    for (int k = 0; k < n_problems; k++) {
        const long long bo = before_range[2 * k], bn = before_range[2 * k + 1], ao = after_range[2 * k], an = after_range[2 * k + 1];
        if (bo < 0 || ao < 0 || bn < 1 || an < 1 || bo + bn > 0x7fffffffLL || ao + an > 0x7fffffffLL) {
            set_error("mi_icp_register_batch: problem %d has an invalid range (before %lld + %lld, after %lld + %lld)", k, bo, bn, ao, an);
            return MI_ERR_INVALID_ARG;
        }
        if (!mi_icp_batch_route((int)bn, (int)an, params)) { fallback.push_back(k); continue; }
        batched.push_back(k);
        span.add(bo, bn, ao, an);
        IcpBatchProblem p{};
        p.b_off = (int)bo; p.n = (int)bn; p.a_off = (int)ao; p.m = (int)an; p.s_off = (int)slots;
        table.push_back(p);
        slots += bn;
        max_pairs = std::max(max_pairs, bn * an);
        if (slots > 0x7fffffffLL) { set_error("mi_icp_register_batch: more than 2^31 moving points in one call (problem %d)", k); return MI_ERR_INVALID_ARG; }
    }
    MI_ENTER(c);
    c->prob.icp_loaded = false;                               // whatever mi_icp_load left is gone, as after mi_icp_register of another pair
    int launches = 0;
    if (!batched.empty()) {
        const int nb = (int)batched.size();
        for (IcpBatchProblem& p : table) { p.b_off -= (int)span.b_lo; p.a_off -= (int)span.a_lo; }
        MI_TRY(c->bat.sx.reserve((size_t)slots)); MI_TRY(c->bat.sy.reserve((size_t)slots)); MI_TRY(c->bat.sz.reserve((size_t)slots));
        MI_TRY(c->bat.problems.reserve((size_t)nb)); MI_TRY(c->bat.states.reserve((size_t)nb));
        MI_TRY(batch_upload_clouds(c, before_xyz, after_xyz, span));
        MI_HIP(hipMemcpyAsync(c->bat.problems.p, table.data(), sizeof(IcpBatchProblem) * (size_t)nb, hipMemcpyHostToDevice, c->stream));
        MI_HIP(hipStreamSynchronize(c->stream));         // (the table is pageable host memory of this frame)
        IcpBatchArgs a{};
        a.before = c->bat.before.p; a.after = c->bat.after.p; a.problems = c->bat.problems.p;
        a.sx = c->bat.sx.p; a.sy = c->bat.sy.p; a.sz = c->bat.sz.p;
        a.states = c->bat.states.p; a.running = c->bat.running.p;
        a.n_problems = nb;
        // a launch ends after `iters` iterations of its longest problem: ~1e9 pair evaluations per workgroup and launch at the most (a few ms),
        // never fewer than 8 iterations (a launch boundary is a host round trip)
        a.iters = (int)std::max(8LL, std::min(64LL, (1LL << 30) / std::max(1LL, max_pairs)));
        a.compose_mode = params->compose_mode;
        a.max_distance_squared = params->max_distance_squared;
        a.rules = icp_rules(*params, 0, c->tune.svd_ieee);   // (sum_mode is MI_SUM_EXACT for every batched problem: mi_icp_batch_route)
        MI_HIP(icp_batch_prepare(a, c->stream));
        MI_TRY(batch_run_until_quiet(c, params->max_iterations != 0, [&] { return icp_batch_iterate(a, params->dist_mode == MI_DIST_FMA, c->stream); }, &launches));
        std::vector<IcpState> states((size_t)nb);
        MI_HIP(hipMemcpyAsync(states.data(), c->bat.states.p, sizeof(IcpState) * (size_t)nb, hipMemcpyDeviceToHost, c->stream));
        MI_HIP(hipStreamSynchronize(c->stream));
        retire_buffers(c);
        for (int i = 0; i < nb; i++) {
            const int k = batched[(size_t)i];
            state_to_outputs(&states[(size_t)i], out_T + 16 * (size_t)k, iterations + k, error + k, stop_reason + k);
        }
    }
    for (int k : fallback) {                             // the existing path, one after the other
        const float* b = before_xyz + 3 * (size_t)before_range[2 * k];
        const float* a = after_xyz + 3 * (size_t)after_range[2 * k];
        MI_TRY(mi_icp_load(c, b, before_range[2 * k + 1], a, after_range[2 * k + 1], params));
        MI_TRY(mi_icp_run(c, -1, nullptr));
        MI_TRY(mi_icp_result(c, out_T + 16 * (size_t)k, iterations + k, error + k, stop_reason + k));
    }
    c->prob.icp_loaded = false;                               // (also what a fallback problem loaded: the call leaves no problem behind, whatever its mix)
    if (info) { info->problems_batched = (int)batched.size(); info->problems_fallback = (int)fallback.size(); info->launches = launches; }
    return MI_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// test-grade primitives
// ---------------------------------------------------------------------------------------------------------------
// Shared set-up of mi_kabsch / mi_transform_mse: source -> (b, c), target -> tgt4, caller's correspondences -> keys.
static int load_pairs(mi_ctx* c, const float* src_xyz, int n, const float* tgt_xyz, int m, const int* idx, const unsigned char* keep)
{
    MI_ENTER(c);
    c->prob.icp_loaded = false;
    if (c->world != 1) { set_error("this primitive is single-GPU only"); return MI_ERR_STATE; }
    for (int i = 0; idx && i < n; i++)
        if (idx[i] < 0 || idx[i] >= m) { set_error("correspondence idx[%d] = %d outside [0,%d)", i, idx[i], m); return MI_ERR_INVALID_ARG; }
    c->prob.n = n;
    c->prob.n_pad = round_up(n, NN_SRC_PAD);
    MI_TRY(reserve_moving(c, (size_t)c->prob.n_pad, (size_t)c->prob.n_pad));
    MI_TRY(reserve_rows(c));
    MI_TRY(upload_soa(c, src_xyz, n, c->prob.n_pad, c->bx.p, c->by.p, c->bz.p, nullptr));
    MI_TRY(copy_before_to_current(c));
    if (tgt_xyz && m > 0) MI_TRY(upload_target_shard(c, tgt_xyz, m));
    else { c->prob.m_total = 0; c->prob.shard_lo = c->prob.shard_hi = 0; MI_TRY(c->tgt4.reserve(1)); }
    if (idx) {
        MI_TRY(c->idx_tmp.reserve((size_t)n));
        MI_HIP(hipMemcpyAsync(c->idx_tmp.p, idx, sizeof(int) * (size_t)n, hipMemcpyHostToDevice, c->stream));
        if (keep) {
            MI_TRY(c->keep_tmp.reserve((size_t)n));
            MI_HIP(hipMemcpyAsync(c->keep_tmp.p, keep, (size_t)n, hipMemcpyHostToDevice, c->stream));
        }
        MI_HIP(pack_keys(c->idx_tmp.p, keep ? c->keep_tmp.p : nullptr, n, c->keys.p, c->stream));
    } else {
        MI_HIP(fill_keys(c->keys.p, n, c->stream));   // index 0xFFFFFFFF is outside every shard: no pair is used
    }
    mi_icp_params_default(&c->prob.icp);
    c->prob.icp.filter_pairs = 1;                       // keys carry d2 = 0 (kept) or +inf (dropped)
    c->prob.icp.max_distance_squared = 1.f;
    state_identity(c->h_state);
    return MI_OK;
}

extern "C" int mi_kabsch(mi_ctx* c, const float* src_xyz, int n, const float* tgt_xyz, int m, const int* idx,
                         const unsigned char* keep, float out_R9[9], float out_t3[3], int* pairs_used)
{
    if (!c || !src_xyz || !tgt_xyz || !idx || n <= 0 || m <= 0 || !out_R9 || !out_t3) { set_error("mi_kabsch: bad arguments"); return MI_ERR_INVALID_ARG; }
    MI_TRY(load_pairs(c, src_xyz, n, tgt_xyz, m, idx, keep));
    MI_HIP(hipMemcpyAsync(c->d_state, c->h_state, sizeof(IcpState), hipMemcpyHostToDevice, c->stream));
    const IcpView v = make_view(c);
    const int nrows = icp_row_count(n);
    { ProfScope ps(c, MI_KERNEL_MOMENTS); MI_HIP(icp_moments_rows(v, c->rows.p, c->stream)); }
    {
        ProfScope ps(c, MI_KERNEL_SOLVE);
        MI_HIP(icp_rows_reduce(c->rows.p, nrows, c->rows_reduced.p, c->stream));
        const IcpRules rules = icp_rules(mi_icp_params{}, 0, c->tune.svd_ieee);     // no stop rule: all zero but the context's MISLAM_SVD_IEEE switch, which holds here as in every other solve
        MI_HIP(icp_solve_deferred(c->d_state, c->rows_reduced.p, icp_reduced_count(nrows), MI_COMPOSE_EXACT, rules, 0, c->stream));
    }
    MI_TRY(icp_fetch_state(c));
    if (pairs_used) *pairs_used = c->h_state->pairs;
    if (c->h_state->pairs <= 0) { set_error("mi_kabsch: no pair kept"); return MI_ERR_INVALID_ARG; }
    memcpy(out_R9, c->h_state->Ri, sizeof(float) * 9);
    memcpy(out_t3, c->h_state->ti, sizeof(float) * 3);
    return MI_OK;
}

extern "C" int mi_cross_moments(mi_ctx* c, const float* src_xyz, int n, const float* tgt_xyz, int m, const int* idx,
                                const unsigned char* keep, double out16[16])
{
    if (!c || !src_xyz || !tgt_xyz || !idx || n <= 0 || m <= 0 || !out16) { set_error("mi_cross_moments: bad arguments"); return MI_ERR_INVALID_ARG; }
    MI_TRY(load_pairs(c, src_xyz, n, tgt_xyz, m, idx, keep));
    MI_HIP(hipMemcpyAsync(c->d_state, c->h_state, sizeof(IcpState), hipMemcpyHostToDevice, c->stream));
    const IcpView v = make_view(c);
    const int nrows = icp_row_count(n);
    { ProfScope ps(c, MI_KERNEL_MOMENTS); MI_HIP(icp_moments_rows(v, c->rows.p, c->stream)); }
    MI_HIP(icp_rows_reduce(c->rows.p, nrows, c->rows_reduced.p, c->stream));
    MI_HIP(icp_rows_to_state(c->d_state, c->rows_reduced.p, icp_reduced_count(nrows), 1, c->stream));
    MI_TRY(icp_fetch_state(c));
    for (int i = 0; i < ICP_MOMENTS; i++) out16[i] = c->h_state->mom[i];
    return MI_OK;
}

extern "C" int mi_transform_mse(mi_ctx* c, const float* src_xyz, int n, const float R9[9], const float t3[3],
                                const float* tgt_xyz, int m, const int* idx, const unsigned char* keep, int divide_by_pairs,
                                float* out_xyz, float* mse)
{
    if (!c || !src_xyz || n <= 0 || !R9 || !t3) { set_error("mi_transform_mse: bad arguments"); return MI_ERR_INVALID_ARG; }
    if (mse && (!tgt_xyz || !idx || m <= 0)) { set_error("mi_transform_mse: mse needs target cloud and idx"); return MI_ERR_INVALID_ARG; }
    MI_TRY(load_pairs(c, src_xyz, n, tgt_xyz, m, mse ? idx : nullptr, keep));
    memcpy(c->h_state->R, R9, sizeof(float) * 9);
    memcpy(c->h_state->t, t3, sizeof(float) * 3);
    MI_HIP(hipMemcpyAsync(c->d_state, c->h_state, sizeof(IcpState), hipMemcpyHostToDevice, c->stream));
    const IcpView v = make_view(c);
    const int nrows = icp_row_count(n);
    { ProfScope ps(c, MI_KERNEL_TRANSFORM); MI_HIP(icp_transform_error_rows(v, c->rows.p, 0, c->stream)); }
    MI_HIP(icp_rows_reduce(c->rows.p, nrows, c->rows_reduced.p, c->stream));
    MI_HIP(icp_rows_to_state(c->d_state, c->rows_reduced.p, icp_reduced_count(nrows), 2, c->stream));
    if (out_xyz) {
        MI_TRY(c->scratch[0].staging.reserve((size_t)3 * n));
        MI_HIP(soa_to_aos(c->cx.p, c->cy.p, c->cz.p, n, c->scratch[0].staging.p, c->stream));
        MI_HIP(hipMemcpyAsync(out_xyz, c->scratch[0].staging.p, sizeof(float) * 3 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    }
    MI_TRY(icp_fetch_state(c));
    if (mse) {
        const double denom = divide_by_pairs ? c->h_state->err[1] : (double)m;
        *mse = (float)(c->h_state->err[0] / denom);
    }
    return MI_OK;
}
