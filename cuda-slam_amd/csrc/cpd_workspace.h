// The CPD drivers' workspace (mi_ctx::cpd: allocated on first use, kept for the context's life) and the functions that cross their three units:
//   cpd_estep.hip     the workspace, the load, the exact / sequential / truncated E-steps, the M-step, sigma^2_0
//   cpd_fgt_api.hip   the Fast-Gauss-Transform E-step and the K-centre / table entry points
//   cpd_api.hip       the entry points: mi_cpd_register, mi_cpd_register_batch, the primitives, the test read-back
// The host arithmetic all three decide by is cpd_plan.hpp.
#pragma once
#include "context.h"
#include "cpd_fgt.h"
#include "cpd_kernels.h"
#include "cpd_plan.hpp"

namespace mislam {

static_assert(PLAN_CPD_T == CPD_T && PLAN_CPD_MAX_CHUNKS == CPD_MAX_CHUNKS && PLAN_CPD_TRUNC_TILE == CPD_TRUNC_TILE &&
              PLAN_CPD_TRUNC_MAX_BLOCKS == CPD_TRUNC_MAX_BLOCKS && PLAN_ICP_MAX_PARTIAL_BLOCKS == ICP_MAX_PARTIAL_BLOCKS,
              "cpd_plan.hpp restates the kernel headers' constants: the values must agree");

// Buffers of one clustered cloud (FgtClusters, cpd_fgt.h)
struct FgtSide {
    DevBuf<float> dist, xc;
    DevBuf<int> indx, memb, off;
    DevBuf<unsigned char> sweep;   // scratch of the grid-wide sweep (large clouds)
    DevBuf<int> picked, replay_state;             // the sweep's choices; the replay's verdict (fgt_replay_kernel)
    DevBuf<unsigned long long> replay_partial;
    int swept_K = 0;            // the fixed cloud only: centres of the sweep dist/indx currently hold (0 = none); see fgt_kcenter_kernel
    int guess_K = 0;            // the moving cloud only: leading entries of `picked` the last E-step's sweep left -- the next one's guess
    int prelaunched = 0;        // > 0: a replay of that guess (this many centres) is on the stream already, behind the last transform
};

// Fast-Gauss-Transform E-step workspace ("approximation-type" full / hybrid)
struct FgtWork {
    FgtSide y, a;
    DevBuf<float> By, Ba;                // coefficients: [K][pd][1] (moving cloud as sources), [K][pd][4] (fixed cloud as sources)
    DevBuf<float> By_part, Ba_part;      // big cells (round 5): the partial sums of fgt_model_splits workgroups per cell, [Z][K][pd][W]
    DevBuf<float> kt1, v4;               // transform outputs, per split of the cells: [S][n], [S][4][m]
    DevBuf<unsigned char> sort_temp;
    DevBuf<unsigned char> sort_temp_a;   // the fixed side's own scratch when its clustering runs beside the moving side's (round 5)
    DevBuf<unsigned int> mono;
    DevBuf<float> ck;
    DevBuf<int> hpos;
    int p = 0, pd = 0;
};

// The rows of M-step partial sums an E-step's own kernels left in part_x / part_k.  Every E-step that leaves them says so with left(); the
// M-step take()s them (and sums by the stand-alone kernels where there are none); whatever makes them stale drop()s them.
struct CpdSumRows {
    bool fresh = false;
    int rows_x = 0, rows_k = 0;
    void left(int x, int k) { fresh = true; rows_x = x; rows_k = k; }
    void drop() { fresh = false; }
    CpdSumRows take() { const CpdSumRows was = *this; fresh = false; return was; }
};

struct CpdWorkspace {
    FgtWork fgt;
    DevBuf<float> ax, ay, az;            // fixed cloud, SoA
    DevBuf<float> den_part, pt1, p1_part, px_part, p1, px;
    DevBuf<float4> xw4;
    DevBuf<double> part_x, part_k, part_init;
    DevBuf<unsigned char> sig_scratch;   // cpd_sigma2_sequential
    // K7t (cpd_trunc.hip): both clouds along a space-filling curve -- the orders (once per load), the fixed cloud's sorted copy and boxes (once),
    // the moving cloud's current positions in curve order and their boxes (every truncated E-step)
    DevBuf<float> t_ax, t_ay, t_az, t_yx, t_yy, t_yz, t_abox, t_ybox;
    DevBuf<int> t_aorder, t_border;
    MortonScratch t_morton;                   // of both orders, one after the other
    DevBuf<float4> t_xw4;
    bool trunc_ready = false;                 // the orders and the fixed cloud's sorted copy belong to the clouds now loaded
    DevBuf<CpdState> d_state;                 // one block
    CpdState* h_state = nullptr;              // pinned (cpd_workspace_destroy frees it)
    int m = 0, n = 0, m_pad = 0, n_pad = 0;   // n = this rank's share of the fixed cloud
    int n_total = 0;                          // |after| over all ranks
    int svd_ieee = 0;                         // the context's MISLAM_SVD_IEEE switch (set where the workspace is fetched)
    int k_chunks = 1, k_chunk_len = 0, x_chunks = 1, x_chunk_len = 0;
    CpdSumRows sums;
    bool replicated = false;                  // multi-rank context, both clouds held WHOLE on every rank (the FGT modes: they cluster whole clouds)
    // Round 6: ... but the E-step's QUERIES are split over the ranks -- the fixed points the first transform is evaluated at
    // [a_lo, a_hi), the moving points of the second [m_lo, m_hi) (mi_shard_range), the truncated E-step's fixed-cloud tiles [t_lo, t_hi) -- and the
    // M-step's 24 sums are all-reduced as in the exact mode.  Clusterings and coefficient tables stay replicated (small, bit-deterministic).
    bool queries_sharded = false;
    int a_lo = 0, a_hi = 0, m_lo = 0, m_hi = 0;
    mi_cpd_params params{};
    // what mi_selftest_cpd_last reports besides the arrays (host bookkeeping only: nothing on the device depends on it)
    int last_estep = -1;                      // MI_CPD_ROUTE_* of the last E-step enqueued (-1: none, or the caller's arrays of mi_cpd_mstep)
    int last_fused = 0, last_rows_x = 0, last_rows_k = 0, last_reduced = 0;   // the last M-step: rows left by the E-step's own kernels?  how many it summed; through cpd_reduce_sums?
    unsigned long long last_call = 0;         // mi_ctx::entered when the last mi_cpd_register / mi_cpd_mstep returned (0: none yet)
};

// ---- cpd_estep.hip
int cpd_workspace(mi_ctx* c, CpdWorkspace** out);            // the context's workspace, created on first use
void cpd_workspace_destroy(mi_ctx* c);                       // (mi_ctx_destroy)
// Uploads both clouds and sizes every buffer; y starts as a copy of b.  Every piece of cross-call state that belonged to the clouds before is dropped.
int cpd_load(mi_ctx* c, CpdWorkspace* w, const float* before_xyz, int m, const float* after_xyz, int n);
CpdView cpd_view(mi_ctx* c, CpdWorkspace* w);
CpdRules cpd_rules(const mi_cpd_params* p, int m, int n_total, int svd_ieee);
// estep_mode: MI_ESTEP_*, from the caller -- a registration passes its parameters' mode, the stand-alone E-step primitives MI_ESTEP_DEFAULT
// (w->params belongs to the last registration on the context: a primitive must not inherit its summation order)
int cpd_estep_enqueue(mi_ctx* c, CpdWorkspace* w, const CpdView& v, int estep_mode);
int cpd_estep_trunc_enqueue(mi_ctx* c, CpdWorkspace* w, const CpdView& v);          // K7t; v.truncate and v.trunc_log set
int cpd_mstep_enqueue(mi_ctx* c, CpdWorkspace* w, const CpdView& v, const CpdRules& rules, int update_loop_state);
int cpd_init(mi_ctx* c, CpdWorkspace* w, const CpdView& v, const CpdRules& rules, float sigma2_override, int sigma2_mode);
int cpd_fetch(mi_ctx* c, CpdWorkspace* w);                   // the state block into w->h_state, and the wait for it
// A multi-rank context whose ranks have each written elements [lo, hi) of buf[0, n): every rank ends up with all of them, bit for bit.  An
// element-wise unsigned MINIMUM against all-ones moves any bit pattern unchanged (a sum would not: NaN payloads, -0).
int exchange_bits(mi_ctx* c, float4* buf, size_t lo, size_t hi, size_t n);

// ---- cpd_fgt_api.hip
// with_sums: the two post kernels also leave the M-step's x-sums / k-sums (the driver's E-steps; a stand-alone E-step reads P1 / Pt1 / PX back instead)
int cpd_estep_fgt_enqueue(mi_ctx* c, CpdWorkspace* w, const CpdView& v, float weight, float sigma2, float sigma2_init, float ratio_of_far_field,
                          int order, bool with_sums = false);
// Behind the transform that ends an EM iteration: the moving cloud's K-centre sweep replayed from that iteration's choices, before the host has K
int cpd_fgt_prelaunch(mi_ctx* c, CpdWorkspace* w, const CpdView& v);

}  // namespace mislam
