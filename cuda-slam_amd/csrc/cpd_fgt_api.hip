// Rigid CPD, the Fast-Gauss-Transform E-step (ComputePMatrixWithFGT, common/cpdutils.cpp:19-77) as the drivers enqueue it, and the entry points
// that run its pieces alone: K-centre clustering (plain and guided) and the host-side monomial tables.  No kernel here (cpd_fgt.hip has them).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "cpd_workspace.h"

using namespace mislam;

namespace mislam {

static int fgt_tables(mi_ctx* c, FgtWork* f, int p, FgtTables* out)
{
    if (p < 1 || p > FGT_MAX_ORDER) { set_error("FGT: order of truncation %d outside [1, %d]", p, FGT_MAX_ORDER); return MI_ERR_INVALID_ARG; }
    if (f->p != p) {
        std::vector<unsigned int> mono; std::vector<float> ck; std::vector<int> hpos;
        fgt_build_tables(p, mono, ck, hpos);
        const size_t pd = mono.size();
        MI_TRY(f->mono.reserve(pd)); MI_TRY(f->ck.reserve(pd)); MI_TRY(f->hpos.reserve(pd));
        MI_HIP(hipMemcpyAsync(f->mono.p, mono.data(), pd * sizeof(unsigned int), hipMemcpyHostToDevice, c->stream));
        MI_HIP(hipMemcpyAsync(f->ck.p, ck.data(), pd * sizeof(float), hipMemcpyHostToDevice, c->stream));
        MI_HIP(hipMemcpyAsync(f->hpos.p, hpos.data(), pd * sizeof(int), hipMemcpyHostToDevice, c->stream));
        MI_HIP(hipStreamSynchronize(c->stream));                   // the staging vectors die here
        f->p = p; f->pd = (int)pd;
    }
    out->mono = f->mono.p; out->ck = f->ck.p; out->hpos = f->hpos.p; out->p = f->p; out->pd = f->pd;
    return MI_OK;
}

static int fgt_side(mi_ctx* c, FgtWork* f, FgtSide* sd, const float* x, const float* y, const float* z, int n, int K, FgtClusters* out)
{
    MI_TRY(sd->dist.reserve(n)); MI_TRY(sd->indx.reserve(n)); MI_TRY(sd->memb.reserve(n));
    MI_TRY(sd->off.reserve((size_t)K + 1)); MI_TRY(sd->xc.reserve(3 * (size_t)K));
    MI_TRY(f->sort_temp.reserve(std::max<size_t>(fgt_sort_temp_bytes(n), 16)));
    if (n > 16 * 1024) MI_TRY(sd->sweep.reserve(FGT_SWEEP_SCRATCH_BYTES));        // (beyond what one workgroup's registers hold: the cooperative / grid-wide sweeps)
    out->sweep_scratch = n > 16 * 1024 ? sd->sweep.p : nullptr;
    out->coop_sweep = c->tune.fgt_coop_sweep;
    // (picked: never shrunk below what a guess still needs -- reserve() keeps the contents when the capacity suffices, and K only grows
    // within a registration; a reallocation loses the guess, so it is dropped with it)
    if (sd->picked.cap < (size_t)K) sd->guess_K = 0;
    MI_TRY(sd->picked.reserve(std::max<size_t>((size_t)K, 1024))); MI_TRY(sd->replay_state.reserve(1));
    out->picked = sd->picked.p; out->guess = 0; out->replay_partial = nullptr; out->replay_state = sd->replay_state.p;
    out->x = x; out->y = y; out->z = z; out->n = n; out->K = K; out->k_done = 0;
    out->dist = sd->dist.p; out->indx = sd->indx.p;
    out->memb = sd->memb.p; out->off = sd->off.p; out->xc = sd->xc.p;
    return MI_OK;
}

// cl->picked[0 .. guess) holds a guess: size the replay's scratch and arm it (guess < 2: nothing to replay)
static int fgt_arm_replay(FgtSide* sd, FgtClusters* cl, int guess)
{
    const int lim = fgt_replay_limit(guess, cl->K);
    if (lim < 1) return MI_OK;
    MI_TRY(sd->replay_partial.reserve((size_t)lim * (size_t)fgt_replay_waves(cl->n)));
    cl->guess = guess; cl->replay_partial = sd->replay_partial.p;
    return MI_OK;
}

// The replay needs the transformed cloud and the guess, not K; K only grows while the FGT is in use, so the next E-step finds exactly the
// replay it would have launched -- 20 us of work inside the ~25 us the device used to wait for the host.
int cpd_fgt_prelaunch(mi_ctx* c, CpdWorkspace* w, const CpdView& v)
{
    FgtWork* f = &w->fgt;
    f->y.prelaunched = 0;
    if (c->tune.fgt_replay == 0 || f->y.guess_K < 2) return MI_OK;
    FgtClusters cy{};
    MI_TRY(fgt_side(c, f, &f->y, v.yx, v.yy, v.yz, w->m, f->y.guess_K, &cy));
    if (f->y.guess_K < 2) return MI_OK;                 // (fgt_side dropped the guess with a reallocated buffer)
    MI_TRY(fgt_arm_replay(&f->y, &cy, f->y.guess_K));
    MI_HIP(fgt_replay_prelaunch(cy, c->stream));
    f->y.prelaunched = fgt_replay_limit(cy.guess, cy.K);
    return MI_OK;
}

int cpd_estep_fgt_enqueue(mi_ctx* c, CpdWorkspace* w, const CpdView& v, float weight, float sigma2, float sigma2_init,
                          float ratio_of_far_field, int order, bool with_sums)
{
    ProfScope ps(c, MI_KERNEL_CPD_FGT);
    w->sums.drop();                      // P1 / Pt1 / PX come from the transform below, not from the exact E-step's post kernels
    FgtWork* f = &w->fgt;
    if (w->m < 2 || w->n < 2) { set_error("FGT E-step needs at least 2 points per cloud (m=%d, n=%d)", w->m, w->n); return MI_ERR_INVALID_ARG; }
    if (!(sigma2 > 0.f)) { set_error("FGT E-step: sigma2 must be positive"); return MI_ERR_INVALID_ARG; }
    FgtTables t{};
    MI_TRY(fgt_tables(c, f, order, &t));
    const int K = fgt_cluster_count(w->m, w->n, sigma2, sigma2_init);
    if (K < 1 || K > FGT_MAX_CLUSTERS) { set_error("FGT E-step: %d cells outside [1, %d]", K, FGT_MAX_CLUSTERS); return MI_ERR_INVALID_ARG; }
    const float hsigma = fgt_hsigma(sigma2);
    const float ndi = fgt_ndi(sigma2, weight, w->m, w->n);
    FgtClusters cy{}, ca{};
    MI_TRY(fgt_side(c, f, &f->y, v.yx, v.yy, v.yz, w->m, K, &cy));
    MI_TRY(fgt_side(c, f, &f->a, v.ax, v.ay, v.az, w->n, K, &ca));
    MI_TRY(f->By.reserve((size_t)K * t.pd)); MI_TRY(f->Ba.reserve(4 * (size_t)K * t.pd));
    // (big cells: a cell's members over several workgroups -- unless the cloud is one whose cells list their own members, which is one workgroup per cell;
    // decided from n, K and pd ALONE: ADVICE r05 found the fixed side taking the listing path on a re-clustering E-step and the split path on the others,
    // two orders of the same sums, for clouds of at most 32 768 points in cells of 1 024 and more)
    const auto splits = [&](int n_side) {
        if (c->tune.fgt_model_splits == 0) return 1;
        if (c->tune.fgt_lists_in_model != 0 && fgt_lists_rule(n_side, K)) return 1;
        return fgt_model_splits(n_side, K, t.pd);
    };
    const int Zy = splits(w->m), Za = splits(w->n);
    if (Zy > 1) MI_TRY(f->By_part.reserve((size_t)Zy * K * t.pd));
    if (Za > 1) MI_TRY(f->Ba_part.reserve(4 * (size_t)Za * K * t.pd));
    const int Sa = fgt_predict_splits(w->n, K), Sy = fgt_predict_splits(w->m, K);
    MI_TRY(f->kt1.reserve((size_t)Sa * w->n)); MI_TRY(f->v4.reserve(4 * (size_t)Sy * w->m));
    const size_t temp = f->sort_temp.cap;
    // Round 5: the FIXED cloud's clustering (the additional centres of a larger K, its member lists: ~18 us of small launches) depends on nothing the
    // moving side computes -- it runs on the context's auxiliary stream, with its own scratch, while `stream` clusters the moving cloud, builds its
    // model and evaluates it; `stream` waits for it just before the fixed side's model.  (With profiling on everything stays on `stream`, one after
    // the other.)  The fixed cloud does not move: the same K needs no new clustering at all, a larger K only the additional centres
    // (a context created under MISLAM_FGT_RESUME=0 re-clusters from scratch every time; the results must not change by a bit -- tests/test_gpu_fgt.py)
    const bool resume = c->tune.fgt_resume != 0;
    const bool recluster = !resume || f->a.swept_K != K;
    const bool beside = recluster && !c->prof.on && c->aux != nullptr && c->tune.fgt_two_streams != 0;
    struct AuxJoin {                       // every way out joins the auxiliary stream into `stream`
        mi_ctx* c; bool armed;
        ~AuxJoin() { if (armed && hipEventRecord(c->aux_event[1], c->aux) == hipSuccess) (void)hipStreamWaitEvent(c->stream, c->aux_event[1], 0); }
    } aux_join{c, false};
    if (recluster) {
        ca.k_done = resume && f->a.swept_K < K ? f->a.swept_K : 0;
        ca.centers_in_model = 1;
        ca.lists_in_model = c->tune.fgt_lists_in_model;
        if (beside) {
            MI_TRY(f->sort_temp_a.reserve(std::max<size_t>(fgt_sort_temp_bytes(w->n), 16)));
            MI_HIP(hipEventRecord(c->aux_event[0], c->stream));                 // behind the last readers of the fixed side's lists
            MI_HIP(hipStreamWaitEvent(c->aux, c->aux_event[0], 0));
            aux_join.armed = true;
            MI_HIP(fgt_cluster(ca, f->sort_temp_a.p, f->sort_temp_a.cap, c->aux));
        }
    }
    // Kt1 = K^T 1: sources = moving cloud, unit weights, queried at the fixed cloud   (cpdutils.cpp:42-43)
    // (the moving cloud's sweep: last E-step's choices replayed and checked in parallel, MISLAM_FGT_REPLAY=0: swept step by step every time)
    MI_TRY(fgt_arm_replay(&f->y, &cy, c->tune.fgt_replay != 0 ? f->y.guess_K : 0));
    // (prelaunched: the same replay went onto the stream behind the last transform, cpd_fgt_prelaunch above -- K has not shrunk below the guess)
    cy.replay_done = f->y.prelaunched > 0 && f->y.prelaunched == fgt_replay_limit(cy.guess, cy.K) ? 1 : 0;
    f->y.prelaunched = 0;
    cy.centers_in_model = 1;                 // (round 5: the cell means come out of the model kernel -- one launch less per side)
    cy.lists_in_model = c->tune.fgt_lists_in_model;      // (... and so do the member lists, for clouds of at most 32 768 points: three launches less per side)
    MI_HIP(fgt_cluster(cy, f->sort_temp.p, temp, c->stream));
    f->y.guess_K = K;
    MI_HIP(fgt_model(cy, nullptr, hsigma, t, f->By.p, c->stream, true, Zy > 1 ? f->By_part.p : nullptr, Zy));
    // The two evaluation kernels carry the E-step's arithmetic and each query is independent of every other: on a multi-rank
    // context a rank evaluates ITS queries only -- with the whole cloud's number of cell splits (Sa, Sy), so that a point's partial sums are grouped as on
    // one GPU and its value is the single-GPU run's to the last bit.
    const bool sharded = w->queries_sharded && with_sums;
    const int a0 = sharded ? w->a_lo : 0, an = sharded ? w->a_hi - w->a_lo : w->n;
    const int m0 = sharded ? w->m_lo : 0, mn = sharded ? w->m_hi - w->m_lo : w->m;
    MI_HIP(fgt_predict(v.ax + a0, v.ay + a0, v.az + a0, an, cy.xc, f->By.p, K, 1, hsigma, ratio_of_far_field, t, Sa, f->kt1.p, c->stream));
    const int nxb = cpd_standalone_sum_blocks(an), nkb = cpd_standalone_sum_blocks(mn);
    MI_HIP(fgt_post_kt1(f->kt1.p, Sa, v.ax + a0, v.ay + a0, v.az + a0, an, ndi, v.pt1 + a0, v.xw4 + a0, c->stream, with_sums ? w->part_x.p : nullptr, nxb));
    // The fixed side's model build weighs EVERY fixed point by its 1/den, x/den (xw4): each rank has written its own range; the others' arrive
    // through the transport, so every rank ends up with the bits the single-GPU run has, and builds the same table from them.
    if (sharded) MI_TRY(exchange_bits(c, v.xw4, (size_t)w->a_lo, (size_t)w->a_hi, (size_t)w->n));
    // P1 and PX: sources = fixed cloud weighted by 1/den and x/den, queried at the moving cloud   (:54-66; the reference
    // clusters the fixed cloud four times with the same result -- once is enough)
    if (recluster) {
        if (beside) {
            MI_HIP(hipEventRecord(c->aux_event[1], c->aux));
            MI_HIP(hipStreamWaitEvent(c->stream, c->aux_event[1], 0));
            aux_join.armed = false;
        } else
            MI_HIP(fgt_cluster(ca, f->sort_temp.p, temp, c->stream));
        f->a.swept_K = K;
    }
    MI_HIP(fgt_model(ca, v.xw4, hsigma, t, f->Ba.p, c->stream, recluster, Za > 1 ? f->Ba_part.p : nullptr, Za));      // (an unchanged clustering keeps its means)
    MI_HIP(fgt_predict(v.yx + m0, v.yy + m0, v.yz + m0, mn, ca.xc, f->Ba.p, K, 4, hsigma, ratio_of_far_field, t, Sy, f->v4.p, c->stream));
    MI_HIP(fgt_post_px(f->v4.p, Sy, mn, v.p1 + m0, v.px + 3 * (size_t)m0, c->stream, with_sums ? w->part_k.p : nullptr, nkb, v.bx + m0, v.by + m0, v.bz + m0));
    if (with_sums) w->sums.left(nxb, nkb);
    w->last_estep = MI_CPD_ROUTE_FGT;
    return MI_OK;
}

// The body of both K-centre entry points.  guided: the caller's guess goes into `picked` and is replayed and checked, the replay's verdict
// and the sweep's choices are read back; the plain call enqueues none of that.
struct KcenterGuide { const int* guess; int n_guess; int* picked; int* verified; };
static int kcenter_run(mi_ctx* c, const float* cloud_xyz, int n, int K, const KcenterGuide* guide, float* centers_xyz, int* cluster)
{
    MI_ENTER(c);
    CpdWorkspace* w = nullptr;
    MI_TRY(cpd_workspace(c, &w));
    c->prob.icp_loaded = false;
    w->fgt.y.guess_K = 0;                // (the buffers of the moving side now hold another cloud's sweep)
    const int n_pad = round_up(n, NN_SRC_PAD);
    MI_TRY(c->bx.reserve(n_pad)); MI_TRY(c->by.reserve(n_pad)); MI_TRY(c->bz.reserve(n_pad));
    MI_TRY(upload_soa(c, cloud_xyz, n, n_pad, c->bx.p, c->by.p, c->bz.p, nullptr));
    FgtClusters cl{};
    MI_TRY(fgt_side(c, &w->fgt, &w->fgt.y, c->bx.p, c->by.p, c->bz.p, n, K, &cl));
    if (guide) {
        const int g = std::min(guide->n_guess, K);
        if (g > 0) MI_HIP(hipMemcpyAsync(cl.picked, guide->guess, sizeof(int) * (size_t)g, hipMemcpyHostToDevice, c->stream));
        MI_HIP(hipMemsetAsync(cl.replay_state, 0xff, sizeof(int), c->stream));            // (-1: no replay ran)
        MI_TRY(fgt_arm_replay(&w->fgt.y, &cl, g));
    }
    MI_HIP(fgt_cluster(cl, w->fgt.sort_temp.p, w->fgt.sort_temp.cap, c->stream));
    MI_HIP(hipMemcpyAsync(cluster, cl.indx, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    MI_HIP(hipMemcpyAsync(centers_xyz, cl.xc, sizeof(float) * 3 * (size_t)K, hipMemcpyDeviceToHost, c->stream));
    int state = -1;
    if (guide) {
        if (guide->picked) MI_HIP(hipMemcpyAsync(guide->picked, cl.picked, sizeof(int) * (size_t)K, hipMemcpyDeviceToHost, c->stream));
        MI_HIP(hipMemcpyAsync(&state, cl.replay_state, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    }
    MI_HIP(hipStreamSynchronize(c->stream));
    if (guide && guide->verified) *guide->verified = state;
    return MI_OK;
}

}  // namespace mislam

extern "C" int mi_fgt_kcenter(mi_ctx* c, const float* cloud_xyz, int n, int K, float* centers_xyz, int* cluster)
{
    if (!c) { set_error("mi_fgt_kcenter: null context"); return MI_ERR_INVALID_ARG; }
    if (!cloud_xyz || !centers_xyz || !cluster) { set_error("mi_fgt_kcenter: null argument"); return MI_ERR_INVALID_ARG; }
    if (n < 2 || K < 1 || K > FGT_MAX_CLUSTERS) { set_error("mi_fgt_kcenter: need n >= 2 and 1 <= K <= %d (n=%d, K=%d)", FGT_MAX_CLUSTERS, n, K); return MI_ERR_INVALID_ARG; }
    return kcenter_run(c, cloud_xyz, n, K, nullptr, centers_xyz, cluster);
}

extern "C" int mi_fgt_kcenter_guided(mi_ctx* c, const float* cloud_xyz, int n, int K, const int* guess, int n_guess, float* centers_xyz, int* cluster,
                                     int* picked, int* verified)
{
    if (!c) { set_error("mi_fgt_kcenter_guided: null context"); return MI_ERR_INVALID_ARG; }
    if (!cloud_xyz || !centers_xyz || !cluster || (n_guess > 0 && !guess)) { set_error("mi_fgt_kcenter_guided: null argument"); return MI_ERR_INVALID_ARG; }
    if (n < 2 || K < 1 || K > FGT_MAX_CLUSTERS || n_guess < 0) { set_error("mi_fgt_kcenter_guided: need n >= 2, 1 <= K <= %d, n_guess >= 0 (n=%d, K=%d, n_guess=%d)", FGT_MAX_CLUSTERS, n, K, n_guess); return MI_ERR_INVALID_ARG; }
    for (int i = 0; i < n_guess; i++)
        if (guess[i] < 0 || guess[i] >= n) { set_error("mi_fgt_kcenter_guided: guess[%d] = %d is not a point of the cloud", i, guess[i]); return MI_ERR_INVALID_ARG; }
    const KcenterGuide guide{guess, n_guess, picked, verified};
    return kcenter_run(c, cloud_xyz, n, K, &guide, centers_xyz, cluster);
}

// Host-only: the monomial tables the FGT kernels use (exponents a | b<<8 | c<<16, C_k, Horner slot), for the CPU-side tests.
extern "C" int mi_fgt_tables(int order_of_truncation, unsigned int* mono, float* ck, int* horner_slot, int* pd_out)
{
    if (order_of_truncation < 1 || order_of_truncation > FGT_MAX_ORDER) { set_error("mi_fgt_tables: order outside [1, %d]", FGT_MAX_ORDER); return MI_ERR_INVALID_ARG; }
    std::vector<unsigned int> m; std::vector<float> k; std::vector<int> h;
    fgt_build_tables(order_of_truncation, m, k, h);
    if (pd_out) *pd_out = (int)m.size();
    if (mono) memcpy(mono, m.data(), m.size() * sizeof(unsigned int));
    if (ck) memcpy(ck, k.data(), k.size() * sizeof(float));
    if (horner_slot) memcpy(horner_slot, h.data(), h.size() * sizeof(int));
    return MI_OK;
}
