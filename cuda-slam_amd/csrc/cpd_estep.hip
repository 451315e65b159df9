// Rigid CPD, the part every caller shares: the workspace, the load, the exact / sequential / truncated E-step enqueues, the M-step with its
// all-reduce and sigma^2_0.  No kernel here: everything is enqueued on the context's stream through cpd_kernels.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "cpd_workspace.h"

namespace mislam {

void cpd_workspace_destroy(mi_ctx* c)
{
    CpdWorkspace* w = c->cpd;
    if (!w) return;
    if (w->h_state) (void)hipHostFree(w->h_state);
    delete w;
    c->cpd = nullptr;
}

int cpd_workspace(mi_ctx* c, CpdWorkspace** out)
{
    if (!c->cpd) {
        c->cpd = new CpdWorkspace();
        MI_TRY(c->cpd->d_state.reserve(1));
        MI_HIP(hipHostMalloc((void**)&c->cpd->h_state, sizeof(CpdState), hipHostMallocDefault));
        memset(c->cpd->h_state, 0, sizeof(CpdState));
    }
    c->cpd->svd_ieee = c->tune.svd_ieee;
    *out = c->cpd;
    return MI_OK;
}

// y starts as a copy of b (transformedCloud = cloudBefore, :104).
int cpd_load(mi_ctx* c, CpdWorkspace* w, const float* before_xyz, int m, const float* after_xyz, int n)
{
    w->last_call = 0;        // nothing to read back until a registration or an M-step has finished on these clouds
    c->prob.icp_loaded = false;   // the moving-cloud buffers are shared with the ICP driver
    w->fgt.a.swept_K = 0;    // a new fixed cloud: its clustering starts over
    w->fgt.y.guess_K = 0;    // a new moving cloud: nothing to guess its sweep from
    w->fgt.y.prelaunched = 0;
    w->m = m; w->n = n; w->n_total = n;
    w->trunc_ready = false;
    w->m_pad = round_up(m, NN_SRC_PAD);
    w->n_pad = round_up(n, NN_SRC_PAD);
    const size_t mp = (size_t)w->m_pad, np = (size_t)w->n_pad;
    MI_TRY(c->bx.reserve(mp)); MI_TRY(c->by.reserve(mp)); MI_TRY(c->bz.reserve(mp));
    MI_TRY(c->cx.reserve(mp)); MI_TRY(c->cy.reserve(mp)); MI_TRY(c->cz.reserve(mp));
    MI_TRY(w->ax.reserve(np)); MI_TRY(w->ay.reserve(np)); MI_TRY(w->az.reserve(np));
    const CpdChunkPlan plan = cpd_chunk_plan(c->cu_count, m, n);
    w->k_chunks = plan.k_chunks; w->k_chunk_len = plan.k_chunk_len;
    w->x_chunks = plan.x_chunks; w->x_chunk_len = plan.x_chunk_len;
    MI_TRY(w->den_part.reserve((size_t)w->k_chunks * n));
    MI_TRY(w->pt1.reserve(np));
    MI_TRY(w->xw4.reserve(np));
    MI_TRY(w->p1_part.reserve((size_t)w->x_chunks * m));
    MI_TRY(w->px_part.reserve((size_t)w->x_chunks * 3 * m));
    MI_TRY(w->p1.reserve(mp));
    MI_TRY(w->px.reserve(3 * mp));
    MI_TRY(w->part_x.reserve((size_t)std::max(ICP_MAX_PARTIAL_BLOCKS, CPD_TRUNC_MAX_BLOCKS) * CPD_XSUMS));
    MI_TRY(w->part_k.reserve((size_t)std::max(ICP_MAX_PARTIAL_BLOCKS, CPD_TRUNC_MAX_BLOCKS) * CPD_KSUMS));
    MI_TRY(w->part_init.reserve((size_t)ICP_MAX_PARTIAL_BLOCKS * CPD_INIT_SUMS));
    MI_TRY(upload_soa(c, before_xyz, m, w->m_pad, c->bx.p, c->by.p, c->bz.p, nullptr));
    MI_TRY(upload_soa(c, after_xyz, n, w->n_pad, w->ax.p, w->ay.p, w->az.p, nullptr));
    const size_t bytes = sizeof(float) * mp;
    MI_HIP(hipMemcpyAsync(c->cx.p, c->bx.p, bytes, hipMemcpyDeviceToDevice, c->stream));
    MI_HIP(hipMemcpyAsync(c->cy.p, c->by.p, bytes, hipMemcpyDeviceToDevice, c->stream));
    MI_HIP(hipMemcpyAsync(c->cz.p, c->bz.p, bytes, hipMemcpyDeviceToDevice, c->stream));
    return MI_OK;
}

CpdView cpd_view(mi_ctx* c, CpdWorkspace* w)
{
    CpdView v{};
    v.state = w->d_state.p;
    v.bx = c->bx.p; v.by = c->by.p; v.bz = c->bz.p;
    v.yx = c->cx.p; v.yy = c->cy.p; v.yz = c->cz.p;
    v.m = w->m;
    v.ax = w->ax.p; v.ay = w->ay.p; v.az = w->az.p;
    v.n = w->n;
    v.den_part = w->den_part.p; v.xw4 = w->xw4.p; v.pt1 = w->pt1.p;
    v.p1_part = w->p1_part.p; v.px_part = w->px_part.p; v.p1 = w->p1.p; v.px = w->px.p;
    v.k_chunks = w->k_chunks; v.k_chunk_len = w->k_chunk_len;
    v.x_chunks = w->x_chunks; v.x_chunk_len = w->x_chunk_len;
    return v;
}

CpdRules cpd_rules(const mi_cpd_params* p, int m, int n_total, int svd_ieee)
{
    CpdRules r{};
    r.eps = p->eps;
    r.weight = cpd_clamp_weight(p->weight);
    r.tolerance = p->tolerance;
    r.const_scale = p->const_scale;
    r.max_iterations = p->max_iterations;
    r.m = m; r.n = n_total;
    r.svd_ieee = svd_ieee;
    return r;
}

static int use_mfma_contraction(const mi_ctx* c) { return c->tune.cpd_mfma; }   // MISLAM_CPD_MFMA, read at context creation

int cpd_estep_enqueue(mi_ctx* c, CpdWorkspace* w, const CpdView& v, int estep_mode)
{
    if (estep_mode == MI_ESTEP_CPU_SEQUENTIAL && !v.truncate) {
        // parity mode: cpu-slam's summation order (cpd_kernels.hip); the M-step's sums then come from the stand-alone kernels
        { ProfScope ps(c, MI_KERNEL_CPD_DENOM); MI_HIP(cpd_estep_sequential(v, c->stream)); }
        w->sums.drop();
        w->last_estep = MI_CPD_ROUTE_SEQUENTIAL;
        return MI_OK;
    }
    // the two post kernels also accumulate the M-step's moments of what they have just produced (two launches less per EM iteration)
    const int nxb = cpd_sum_blocks(w->n), nkb = cpd_sum_blocks(w->m);
    { ProfScope ps(c, MI_KERNEL_CPD_DENOM); MI_HIP(cpd_denominators(v, c->stream)); }
    MI_HIP(cpd_post_denominators(v, c->stream, w->part_x.p, nxb));
    { ProfScope ps(c, MI_KERNEL_CPD_CONTRACT); MI_HIP(cpd_contract(v, use_mfma_contraction(c), c->stream)); }
    MI_HIP(cpd_post_contract(v, c->stream, w->part_k.p, nkb));
    w->sums.left(nxb, nkb);
    w->last_estep = v.truncate ? MI_CPD_ROUTE_TRUNC_EVERY_PAIR : use_mfma_contraction(c) ? MI_CPD_ROUTE_EXACT_MFMA : MI_CPD_ROUTE_EXACT_VALU;
    return MI_OK;
}

int exchange_bits(mi_ctx* c, float4* buf, size_t lo, size_t hi, size_t n)
{
    if (lo > 0) MI_HIP(hipMemsetAsync(buf, 0xff, sizeof(float4) * lo, c->stream));
    if (hi < n) MI_HIP(hipMemsetAsync(buf + hi, 0xff, sizeof(float4) * (n - hi), c->stream));
    MI_TRY(allreduce_min_u64(c, reinterpret_cast<unsigned long long*>(buf), 2 * n));
    return MI_OK;
}

// K7t: the hybrid mode's truncated E-step, culled (cpd_trunc.hip).  MISLAM_CPD_TRUNC_CULL=0: round 4's every-pair truncated kernels.
static int cpd_trunc_prepare(mi_ctx* c, CpdWorkspace* w, const CpdView& v)
{
    if (w->trunc_ready) return MI_OK;
    MI_TRY(w->t_aorder.reserve(w->n)); MI_TRY(w->t_border.reserve(w->m));
    const size_t na = (size_t)cpd_trunc_tiles(w->n) * CPD_TRUNC_TILE, ny = (size_t)cpd_trunc_tiles(w->m) * CPD_TRUNC_TILE;
    MI_TRY(w->t_ax.reserve(na)); MI_TRY(w->t_ay.reserve(na)); MI_TRY(w->t_az.reserve(na)); MI_TRY(w->t_xw4.reserve(na));
    MI_TRY(w->t_yx.reserve(ny)); MI_TRY(w->t_yy.reserve(ny)); MI_TRY(w->t_yz.reserve(ny));
    constexpr int per_tile = 1 + CPD_TRUNC_TILE / CPD_TRUNC_GROUP;          // a tile's box + its groups' boxes
    MI_TRY(w->t_abox.reserve(6 * (size_t)per_tile * cpd_trunc_tiles(w->n)));
    MI_TRY(w->t_ybox.reserve(6 * (size_t)per_tile * cpd_trunc_tiles(w->m)));
    // the fixed cloud along its curve; the moving cloud along the curve of its ORIGINAL points (a similarity transform keeps neighbours together)
    // (both sorts out of one scratch, sized for the larger cloud)
    MortonArgs ma{};
    MI_TRY(morton_args(w->t_morton, v.ax, v.ay, v.az, std::max(w->m, w->n), w->t_aorder.p, &ma));
    ma.m = w->n;
    MI_HIP(morton_order(ma, c->stream));
    ma.x = v.bx; ma.y = v.by; ma.z = v.bz; ma.m = w->m; ma.order_out = w->t_border.p;
    MI_HIP(morton_order(ma, c->stream));
    MI_HIP(cpd_trunc_gather(v.ax, v.ay, v.az, w->t_aorder.p, w->n, w->t_ax.p, w->t_ay.p, w->t_az.p, w->t_abox.p,
                            w->t_abox.p + 6 * (size_t)cpd_trunc_tiles(w->n), nullptr, c->stream));
    w->trunc_ready = true;
    return MI_OK;
}

int cpd_estep_trunc_enqueue(mi_ctx* c, CpdWorkspace* w, const CpdView& v)
{
    MI_TRY(cpd_trunc_prepare(c, w, v));
    CpdTruncView t{};
    t.state = v.state;
    t.ax = w->t_ax.p; t.ay = w->t_ay.p; t.az = w->t_az.p;
    t.abox = w->t_abox.p; t.agroup = w->t_abox.p + 6 * (size_t)cpd_trunc_tiles(w->n);
    t.a_order = w->t_aorder.p; t.n = w->n;
    t.yx = w->t_yx.p; t.yy = w->t_yy.p; t.yz = w->t_yz.p;
    t.ybox = w->t_ybox.p; t.ygroup = w->t_ybox.p + 6 * (size_t)cpd_trunc_tiles(w->m);
    t.b_order = w->t_border.p; t.m = w->m;
    t.bx = v.bx; t.by = v.by; t.bz = v.bz;
    t.xw4 = w->t_xw4.p; t.xw4_caller = v.xw4; t.pt1 = v.pt1; t.p1 = v.p1; t.px = v.px;
    t.trunc_log = v.trunc_log;
    // a multi-rank context: this rank's tiles of the FIXED cloud (curve order) for the denominators, its tiles of the MOVING cloud for the contraction, each
    // against the whole other cloud -- per-point values bit for bit the single-GPU run's; the M-step's sums are added over the ranks
    t.a_tile_lo = 0; t.a_tile_hi = cpd_trunc_tiles(w->n); t.y_tile_lo = 0; t.y_tile_hi = cpd_trunc_tiles(w->m);
    if (w->queries_sharded) {
        (void)mi_shard_range(cpd_trunc_tiles(w->n), c->rank, c->world, &t.a_tile_lo, &t.a_tile_hi);
        (void)mi_shard_range(cpd_trunc_tiles(w->m), c->rank, c->world, &t.y_tile_lo, &t.y_tile_hi);
    }
    const int nxb = cpd_trunc_rows(t.a_tile_lo, t.a_tile_hi), nkb = cpd_trunc_rows(t.y_tile_lo, t.y_tile_hi);
    // the moving cloud's current positions in curve order + this E-step's boxes
    MI_HIP(cpd_trunc_gather(v.yx, v.yy, v.yz, w->t_border.p, w->m, w->t_yx.p, w->t_yy.p, w->t_yz.p, w->t_ybox.p,
                            w->t_ybox.p + 6 * (size_t)cpd_trunc_tiles(w->m), v.state, c->stream));
    { ProfScope ps(c, MI_KERNEL_CPD_DENOM); MI_HIP(cpd_trunc_denominators(t, w->part_x.p, nxb, c->stream)); }
    if (w->queries_sharded) {
        // the contraction's operand (w x, w y, w z, w per fixed point, curve order): every rank has written its own tiles' points
        const size_t p_lo = (size_t)t.a_tile_lo * CPD_TRUNC_TILE, p_hi = std::min((size_t)t.a_tile_hi * CPD_TRUNC_TILE, (size_t)w->n);
        MI_TRY(exchange_bits(c, w->t_xw4.p, p_lo, p_hi, (size_t)w->n));
    }
    { ProfScope ps(c, MI_KERNEL_CPD_CONTRACT); MI_HIP(cpd_trunc_contract(t, w->part_k.p, nkb, c->stream)); }
    w->sums.left(nxb, nkb);
    w->last_estep = MI_CPD_ROUTE_TRUNC_CULLED;
    return MI_OK;
}

int cpd_mstep_enqueue(mi_ctx* c, CpdWorkspace* w, const CpdView& v, const CpdRules& rules, int update_loop_state)
{
    ProfScope ps(c, MI_KERNEL_CPD_MSTEP);
    const CpdSumRows left = w->sums.take();
    int nxb = left.rows_x, nkb = left.rows_k;                // (the rows the E-step's own kernels left)
    if (!left.fresh) {
        nxb = cpd_standalone_sum_blocks(w->n); nkb = cpd_standalone_sum_blocks(w->m);
        MI_HIP(cpd_xsums(v, w->part_x.p, nxb, c->stream));
        MI_HIP(cpd_ksums(v, w->part_k.p, nkb, c->stream));
    }
    w->last_fused = left.fresh ? 1 : 0; w->last_rows_x = nxb; w->last_rows_k = nkb;
    w->last_reduced = 0;
    if (!c->distributed() || (w->replicated && !w->queries_sharded)) {
        MI_HIP(cpd_solve(w->d_state.p, w->part_x.p, nxb, w->part_k.p, nkb, rules, update_loop_state, c->stream));
        return MI_OK;
    }
    // Fixed cloud sharded over the ranks (C2): the x-sums cover this rank's fixed points, the k-sums are linear
    // in this rank's share of P1/PX -- ONE all-reduce of the 24 doubles gives every rank the full moments; the per-point P1/PX
    // never travel.  Every rank then runs the same solve.
    static_assert(offsetof(CpdState, ks) == offsetof(CpdState, xs) + sizeof(double) * CPD_XSUMS, "xs and ks must be contiguous");
    MI_HIP(cpd_reduce_sums(w->d_state.p, w->part_x.p, nxb, w->part_k.p, nkb, c->stream));
    w->last_reduced = 1;
    MI_TRY(allreduce_sum_f64(c, w->d_state.p->xs, (size_t)(CPD_XSUMS + CPD_KSUMS)));
    MI_HIP(cpd_solve(w->d_state.p, nullptr, 0, nullptr, 0, rules, update_loop_state, c->stream));
    return MI_OK;
}

int cpd_fetch(mi_ctx* c, CpdWorkspace* w)
{
    MI_HIP(hipMemcpyAsync(w->h_state, w->d_state.p, sizeof(CpdState), hipMemcpyDeviceToHost, c->stream));
    MI_HIP(hipStreamSynchronize(c->stream));
    return MI_OK;
}

int cpd_init(mi_ctx* c, CpdWorkspace* w, const CpdView& v, const CpdRules& rules, float sigma2_override, int sigma2_mode)
{
    const int nb = icp_reduce_blocks(std::max(w->m, w->n));
    MI_HIP(cpd_init_sums(v, w->part_init.p, nb, c->stream));
    const int seq = sigma2_mode == MI_SIGMA2_CPU_SEQUENTIAL && !(sigma2_override > 0.f);
    if (seq) {
        if (c->distributed() && !w->replicated) { set_error("CPD: MI_SIGMA2_CPU_SEQUENTIAL needs a single-GPU context (one running sum over all pairs)"); return MI_ERR_INVALID_ARG; }
        MI_TRY(w->sig_scratch.reserve(cpd_sigma2_scratch_bytes()));
        MI_HIP(cpd_sigma2_sequential(v, c->stream, w->sig_scratch.p, (int*)c->h_scratch));
    }
    if (!c->distributed() || w->replicated) {
        MI_HIP(cpd_init_state(w->d_state.p, w->part_init.p, nb, rules, sigma2_override, seq, c->stream));
        return MI_OK;
    }
    // sharded fixed cloud: its four sums (init[0..3]) are added over the ranks; the moving cloud's (init[4..7]) are replicated
    MI_HIP(cpd_reduce_init(w->d_state.p, w->part_init.p, nb, c->stream));
    MI_TRY(allreduce_sum_f64(c, w->d_state.p->init, 4));
    MI_HIP(cpd_init_state(w->d_state.p, nullptr, 0, rules, sigma2_override, 0, c->stream));
    return MI_OK;
}

}  // namespace mislam
