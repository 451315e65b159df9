// mi_pose_graph_optimize and mi_pose_graph_system behind the C ABI: the argument checks (on the host: the call is host in, host out, and every
// array is walked once anyway for its AoS -> SoA repacking), the reserves of the call's own buffers in the context, the upload, the incidence
// lists by the library's radix sort (K56), and then either the Levenberg-Marquardt loop around the device's inner solve or one linearisation
// stage by stage (K57-K63, pose_graph_kernels.hip).  The host decides accept or reject from the two costs in the state block and reads that
// block once per linearisation, every PG_SYNC_EVERY iterations of a solve and once per candidate -- never per conjugate-gradient iteration.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "context.h"
#include "pose_graph_terms.hpp"

using namespace mislam;

namespace {

constexpr int PG_SYNC_EVERY = 16;             // conjugate-gradient iterations between host reads of the state block
constexpr int PG_MAX_REJECTIONS = 8;
constexpr double PG_LAMBDA_MIN = 1e-12;
constexpr double PG_ORTHOGONAL_TOL = 1e-3;

struct PgInputs {
    const double* poses; int V;
    const int *src, *tgt; const double* edge_T; const double* info; const unsigned char* uncertain; int E;
    const mi_pose_graph_params* p;
};

// a column-major 4 x 4 as 12 numbers (R row-major, then t); false: a non-finite entry or a rotation block too far from orthogonal, *why says which
bool pg_take_transform(const double* T, double (&out)[PG_POSE], const char** why)
{
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) out[3 * i + j] = T[4 * j + i];
        out[9 + i] = T[12 + i];
    }
    for (int i = 0; i < PG_POSE; i++)
        if (!std::isfinite(out[i])) { *why = "has a non-finite entry"; return false; }
    double worst = 0.0;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            const double d = ((out[i] * out[j] + out[3 + i] * out[3 + j]) + out[6 + i] * out[6 + j]) - (i == j ? 1.0 : 0.0);
            if (std::fabs(d) > worst) worst = std::fabs(d);
        }
    if (!(worst <= PG_ORTHOGONAL_TOL)) { *why = "has a rotation block with max |R^T R - I| above 1e-3"; return false; }
    return true;
}

int pg_check_scalars(const char* who, mi_ctx* c, const PgInputs& in)
{
    if (!c) { set_error("%s: null context", who); return MI_ERR_INVALID_ARG; }
    if (!in.poses) { set_error("%s: null poses", who); return MI_ERR_INVALID_ARG; }
    if (!in.p) { set_error("%s: null params", who); return MI_ERR_INVALID_ARG; }
    if (in.V < 1) { set_error("%s: V = %d, no node", who, in.V); return MI_ERR_INVALID_ARG; }
    if (in.E < 0) { set_error("%s: E = %d is negative", who, in.E); return MI_ERR_INVALID_ARG; }
    if (in.E >= (1 << 30)) { set_error("%s: E = %d, beyond the 2^30 - 1 edges the incidence lists index", who, in.E); return MI_ERR_INVALID_ARG; }
    if (in.E > 0 && (!in.src || !in.tgt || !in.edge_T || !in.info)) { set_error("%s: null edge_source, edge_target, edge_T or edge_information", who); return MI_ERR_INVALID_ARG; }
    const mi_pose_graph_params& p = *in.p;
    if (p.reference_node < 0 || p.reference_node >= in.V) { set_error("%s: reference_node %d outside [0, %d)", who, p.reference_node, in.V); return MI_ERR_INVALID_ARG; }
    if (!(p.pcg_tolerance >= 0.0)) { set_error("%s: pcg_tolerance %g is NaN or negative", who, p.pcg_tolerance); return MI_ERR_INVALID_ARG; }
    if (!(p.relative_decrease >= 0.0)) { set_error("%s: relative_decrease %g is NaN or negative", who, p.relative_decrease); return MI_ERR_INVALID_ARG; }
    if (!(p.absolute_cost >= 0.0)) { set_error("%s: absolute_cost %g is NaN or negative", who, p.absolute_cost); return MI_ERR_INVALID_ARG; }
    if (!(p.line_process_mu >= 0.0)) { set_error("%s: line_process_mu %g is NaN or negative", who, p.line_process_mu); return MI_ERR_INVALID_ARG; }
    if (!(p.lambda0 > 0.0) || !std::isfinite(p.lambda0)) { set_error("%s: lambda0 %g is not a positive number", who, p.lambda0); return MI_ERR_INVALID_ARG; }
    return MI_OK;
}

// The arrays' checks and their repacking in one walk: poses12 (12 V, AoS), Z (SoA [12][E]), L (SoA [21][E]), the nodes with long lists.
int pg_check_and_pack(const char* who, const PgInputs& in, std::vector<double>& poses12, std::vector<double>& Z, std::vector<double>& L,
                      std::vector<int>& long_nodes)
{
    const size_t V = (size_t)in.V, E = (size_t)in.E;
    for (size_t e = 0; e < E; e++) {
        if (in.src[e] < 0 || in.src[e] >= in.V) { set_error("%s: edge_source[%zu] = %d outside [0, %d)", who, e, in.src[e], in.V); return MI_ERR_INVALID_ARG; }
        if (in.tgt[e] < 0 || in.tgt[e] >= in.V) { set_error("%s: edge_target[%zu] = %d outside [0, %d)", who, e, in.tgt[e], in.V); return MI_ERR_INVALID_ARG; }
        if (in.src[e] == in.tgt[e]) { set_error("%s: edge_target[%zu] = %d is the edge's own source", who, e, in.tgt[e]); return MI_ERR_INVALID_ARG; }
    }
    poses12.resize(PG_POSE * V);
    const char* why = "";
    double T[PG_POSE];
    for (size_t k = 0; k < V; k++) {
        if (!pg_take_transform(in.poses + 16 * k, T, &why)) { set_error("%s: poses[%zu] %s", who, k, why); return MI_ERR_INVALID_ARG; }
        for (int i = 0; i < PG_POSE; i++) poses12[PG_POSE * k + i] = T[i];
    }
    Z.resize(PG_POSE * E);
    for (size_t e = 0; e < E; e++) {
        if (!pg_take_transform(in.edge_T + 16 * e, T, &why)) { set_error("%s: edge_T[%zu] %s", who, e, why); return MI_ERR_INVALID_ARG; }
        for (int i = 0; i < PG_POSE; i++) Z[(size_t)i * E + e] = T[i];
    }
    L.resize(PG_TRI * E);
    for (size_t e = 0; e < E; e++) {
        const double* I = in.info + 36 * e;
        int k = 0;
        for (int i = 0; i < 6; i++)
            for (int j = i; j < 6; j++) {
                const double v = I[6 * i + j];
                if (!std::isfinite(v)) { set_error("%s: edge_information[%zu] has a non-finite entry (%d, %d)", who, e, i, j); return MI_ERR_INVALID_ARG; }
                if (i == j && v < 0.0) { set_error("%s: edge_information[%zu] has the negative diagonal entry %g at (%d, %d)", who, e, v, i, i); return MI_ERR_INVALID_ARG; }
                L[(size_t)k * E + e] = v;
                k++;
            }
    }
    std::vector<int> degree(V, 0);
    for (size_t e = 0; e < E; e++) { degree[in.src[e]]++; degree[in.tgt[e]]++; }
    long_nodes.clear();
    for (size_t k = 0; k < V; k++)
        if (degree[k] > PG_LONG_LIST) long_nodes.push_back((int)k);
    return MI_OK;
}

struct PgDevice {
    PgGraph g{};
    PgTerms t{}, cand{};
    PgVectors v{};
};

// reserves (stage 0), upload (1), incidence lists (2).  Needs E > 0.
int pg_setup(mi_ctx* c, StageClock& clock, CallBuffers& bufs, const PgInputs& in, const std::vector<double>& poses12, const std::vector<double>& Z,
             const std::vector<double>& L, const std::vector<int>& long_nodes, bool want_p, PgDevice* d)
{
    mi_ctx::PoseGraphBuffers& b = c->pose_graph;
    const size_t V = (size_t)in.V, E = (size_t)in.E, n2 = 2 * E;
    const size_t nb = (size_t)pg_blocks(in.V), eb = (size_t)pg_blocks(in.E), nl = long_nodes.size();
    MI_TRY(bufs.need(b.poses, PG_POSE * V)); MI_TRY(bufs.need(b.candidate, PG_POSE * V));
    MI_TRY(bufs.need(b.src, E)); MI_TRY(bufs.need(b.tgt, E));
    MI_TRY(bufs.need(b.list, n2)); MI_TRY(bufs.need(b.list_tmp, n2)); MI_TRY(bufs.need(b.offsets, V + 1));
    MI_TRY(bufs.need(b.long_nodes, nl > 0 ? nl : 1));
    if (in.uncertain) MI_TRY(bufs.need(b.uncertain, E));
    MI_TRY(bufs.need(b.Z, PG_POSE * E)); MI_TRY(bufs.need(b.L, PG_TRI * E));
    MI_TRY(bufs.need(b.keys_a, n2)); MI_TRY(bufs.need(b.keys_b, n2));
    MI_TRY(bufs.need(b.sort_temp, radix_sort_temp_bytes((int)n2) + 16));
    MI_TRY(bufs.need(b.r, 6 * E)); MI_TRY(bufs.need(b.chi2, E)); MI_TRY(bufs.need(b.w, E)); MI_TRY(bufs.need(b.M, PG_TRI * E)); MI_TRY(bufs.need(b.h, 6 * E));
    MI_TRY(bufs.need(b.chi2_c, E)); MI_TRY(bufs.need(b.w_c, E));
    MI_TRY(bufs.need(b.cost_parts, eb));
    MI_TRY(bufs.need(b.diag, PG_TRI * V)); MI_TRY(bufs.need(b.grad, 6 * V));
    MI_TRY(bufs.need(b.x, 6 * V)); MI_TRY(bufs.need(b.pr, 6 * V)); MI_TRY(bufs.need(b.pz, 6 * V)); MI_TRY(bufs.need(b.pp, 6 * V)); MI_TRY(bufs.need(b.pq, 6 * V));
    MI_TRY(bufs.need(b.pq_node, V)); MI_TRY(bufs.need(b.parts, 2 * nb));
    if (want_p) { MI_TRY(bufs.need(b.user_p, 6 * V)); MI_TRY(bufs.need(b.hp, 6 * V)); }
    MI_TRY(bufs.need(b.state, 1));
    MI_TRY(clock.mark(0));

    MI_TRY(host_to_device(c, b.poses.p, poses12.data(), sizeof(double) * PG_POSE * V));
    MI_TRY(host_to_device(c, b.src.p, in.src, sizeof(int) * E));
    MI_TRY(host_to_device(c, b.tgt.p, in.tgt, sizeof(int) * E));
    MI_TRY(host_to_device(c, b.Z.p, Z.data(), sizeof(double) * PG_POSE * E));
    MI_TRY(host_to_device(c, b.L.p, L.data(), sizeof(double) * PG_TRI * E));
    if (in.uncertain) MI_TRY(host_to_device(c, b.uncertain.p, in.uncertain, E));
    if (nl > 0) MI_TRY(host_to_device(c, b.long_nodes.p, long_nodes.data(), sizeof(int) * nl));
    MI_HIP(hipMemsetAsync(b.state.p, 0, sizeof(PgState), c->stream));
    MI_TRY(clock.mark(1));

    PgGraph& g = d->g;
    g.V = in.V; g.E = in.E; g.reference = in.p->reference_node;
    g.src = b.src.p; g.tgt = b.tgt.p; g.uncertain = in.uncertain ? b.uncertain.p : nullptr;
    g.Z = b.Z.p; g.L = b.L.p; g.long_nodes = b.long_nodes.p; g.n_long = (int)nl; g.mu = in.p->line_process_mu;
    // host-side shape check before the hand-written kernels run: every array they index is as long as the launches assume
    if (!bufs.fits()) { set_error("internal: pose-graph buffers shorter than the launch"); return MI_ERR_STATE; }

    // the 2 E (node, 2 * edge + side) pairs, ordered by node; the sort is stable, so a node's entries stay ascending
    int bits = 10;
    while (bits < 30 && ((long long)1 << bits) < (long long)in.V) bits += 10;
    MI_HIP(pg_incidence_keys(g.src, g.tgt, nullptr, (int)n2, 0, b.keys_a.p, b.list_tmp.p, c->stream));
    MI_HIP(radix_sort_pairs_u32(b.sort_temp.p, b.keys_a.p, b.keys_b.p, b.list_tmp.p, b.list.p, (int)n2, bits, c->stream));
    g.list = b.list.p;
    if ((long long)in.V > ((long long)1 << 30)) {              // the node's bit 30, behind the 30 below it
        MI_HIP(pg_incidence_keys(g.src, g.tgt, b.list.p, (int)n2, 30, b.keys_a.p, nullptr, c->stream));
        MI_HIP(radix_sort_pairs_u32(b.sort_temp.p, b.keys_a.p, b.keys_b.p, b.list.p, b.list_tmp.p, (int)n2, 10, c->stream));
        g.list = b.list_tmp.p;
    }
    MI_HIP(pg_build_offsets(g, b.offsets.p, c->stream));
    g.offsets = b.offsets.p;
    MI_TRY(clock.mark(2));

    d->t = PgTerms{b.r.p, b.chi2.p, b.w.p, b.M.p, b.h.p};
    d->cand = PgTerms{b.r.p, b.chi2_c.p, b.w_c.p, b.M.p, b.h.p};   // (the candidate pass writes chi2 and w alone)
    d->v = PgVectors{b.x.p, b.pr.p, b.pz.p, b.pp.p, b.pq.p, b.pq_node.p, b.parts.p};
    return MI_OK;
}

int pg_read_state(mi_ctx* c, PgState* h)
{
    MI_HIP(hipMemcpyAsync(c->h_scratch, c->pose_graph.state.p, sizeof(PgState), hipMemcpyDeviceToHost, c->stream));
    MI_HIP(hipStreamSynchronize(c->stream));
    std::memcpy(h, c->h_scratch, sizeof(PgState));
    return MI_OK;
}

int pg_linearise(mi_ctx* c, const PgDevice& d, const double* poses)
{
    mi_ctx::PoseGraphBuffers& b = c->pose_graph;
    MI_HIP(pg_edge_terms_launch(d.g, poses, d.t, 1, b.cost_parts.p, c->stream));
    MI_HIP(pg_cost_finish(b.cost_parts.p, pg_blocks(d.g.E), b.state.p, 0, c->stream));
    MI_HIP(pg_node_gather(d.g, d.t, b.diag.p, b.grad.p, c->stream));
    return MI_OK;
}

// the inner solve at `lambda`, to its stop: *h is the state behind it
int pg_solve(mi_ctx* c, const char* who, const PgDevice& d, double lambda, const mi_pose_graph_params& p, PgState* h)
{
    mi_ctx::PoseGraphBuffers& b = c->pose_graph;
    MI_HIP(pg_pcg_begin(d.g, b.diag.p, b.grad.p, lambda, p.pcg_tolerance, p.max_pcg_iterations, d.v, b.state.p, c->stream));
    int enqueued = 0;
    for (;;) {
        const int todo = p.max_pcg_iterations - enqueued < PG_SYNC_EVERY ? p.max_pcg_iterations - enqueued : PG_SYNC_EVERY;
        if (todo > 0) MI_HIP(pg_pcg_iterations(d.g, d.t, b.diag.p, lambda, d.v, b.state.p, todo, c->stream));
        enqueued += todo > 0 ? todo : 0;
        MI_TRY(pg_read_state(c, h));
        if (h->done) return MI_OK;
        if (todo <= 0) { set_error("internal: %s ran %d conjugate-gradient iterations without a stop", who, enqueued); return MI_ERR_STATE; }
    }
}

void pg_transpose_out(const std::vector<double>& soa, size_t count, int width, double* out)
{
    for (size_t i = 0; i < count; i++)
        for (int c = 0; c < width; c++) out[(size_t)width * i + c] = soa[(size_t)c * count + i];
}

int pg_download_soa(mi_ctx* c, const double* dev, size_t count, int width, std::vector<double>& host)
{
    host.resize((size_t)width * count);
    MI_HIP(hipMemcpyAsync(host.data(), dev, sizeof(double) * host.size(), hipMemcpyDeviceToHost, c->stream));
    return MI_OK;
}

}  // namespace

extern "C" void mi_pose_graph_default_params(mi_pose_graph_params* p)
{
    if (!p) return;
    p->max_iterations = 50; p->max_pcg_iterations = 200; p->reference_node = 0;
    p->pcg_tolerance = 1e-8; p->relative_decrease = 1e-9; p->absolute_cost = 0.0; p->lambda0 = 1e-6; p->line_process_mu = 0.0;
}

extern "C" int mi_pose_graph_optimize(mi_ctx* c, const double* poses, int V, const int* edge_source, const int* edge_target, const double* edge_T,
                                      const double* edge_information, const unsigned char* edge_uncertain, int E, const mi_pose_graph_params* params,
                                      double* out_poses, double* out_weights, double* out_chi2, double out_report[8])
{
    const char* who = "mi_pose_graph_optimize";
    const PgInputs in{poses, V, edge_source, edge_target, edge_T, edge_information, edge_uncertain, E, params};
    MI_TRY(pg_check_scalars(who, c, in));
    if (!out_poses || !out_report) { set_error("%s: null out_poses or out_report", who); return MI_ERR_INVALID_ARG; }
    std::vector<double> poses12, Z, L;
    std::vector<int> long_nodes;
    MI_TRY(pg_check_and_pack(who, in, poses12, Z, L, long_nodes));
    if (c->distributed()) { set_error("%s: single-GPU contexts only", who); return MI_ERR_STATE; }
    MI_ENTER(c);
    mi_ctx::PoseGraphBuffers& b = c->pose_graph;
    StageClock clock(c, b.ms);         // mi_pose_graph_times
    const mi_pose_graph_params& p = *params;
    const size_t Vn = (size_t)V;

    double report[8] = {0.0, 0.0, 0.0, 0.0, 0.0, p.lambda0, (double)MI_STOP_CONVERGED, 0.0};
    if (E == 0) {                      // nothing constrains anything: the poses as given
        if (out_poses != poses) std::memmove(out_poses, poses, sizeof(double) * 16 * Vn);
        for (int i = 0; i < 8; i++) out_report[i] = report[i];
        clock.finish();
        return MI_OK;
    }

    CallBuffers bufs;
    PgDevice d;
    MI_TRY(pg_setup(c, clock, bufs, in, poses12, Z, L, long_nodes, false, &d));

    double* cur = b.poses.p;
    double* cand = b.candidate.p;
    PgState h{};
    MI_TRY(pg_linearise(c, d, cur));
    MI_TRY(pg_read_state(c, &h));
    MI_TRY(clock.mark(3));
    double F = h.cost[0], lambda = p.lambda0;
    int linearisations = 1, accepted = 0, rejections = 0, stop = MI_STOP_RUNNING;
    long long pcg_total = 0;
    double last_rel = 0.0;
    bool final_is_candidate = false;  // which arrays hold chi2 and w at the returned poses
    report[0] = F;
    if (F <= p.absolute_cost) stop = MI_STOP_CONVERGED;
    else if (p.max_iterations < 1) stop = MI_STOP_MAX_ITERATIONS;
    while (stop == MI_STOP_RUNNING) {
        MI_TRY(pg_solve(c, who, d, lambda, p, &h));
        pcg_total += h.iterations;
        last_rel = h.gg > 0.0 ? std::sqrt(h.rr) / std::sqrt(h.gg) : 0.0;
        MI_TRY(clock.mark(4));
        MI_HIP(pg_apply_step(d.g, cur, d.v.x, cand, c->stream));
        MI_HIP(pg_edge_terms_launch(d.g, cand, d.cand, 0, b.cost_parts.p, c->stream));
        MI_HIP(pg_cost_finish(b.cost_parts.p, pg_blocks(E), b.state.p, 1, c->stream));
        MI_TRY(pg_read_state(c, &h));
        MI_TRY(clock.mark(5));
        const double F_new = h.cost[1];
        if (F_new < F) {
            double* tmp = cur; cur = cand; cand = tmp;
            accepted++; rejections = 0;
            lambda = lambda / 10.0 > PG_LAMBDA_MIN ? lambda / 10.0 : PG_LAMBDA_MIN;
            const double decrease = (F - F_new) / F;
            F = F_new;
            final_is_candidate = true;
            if (decrease <= p.relative_decrease || F <= p.absolute_cost) stop = MI_STOP_CONVERGED;
            else if (linearisations >= p.max_iterations) stop = MI_STOP_MAX_ITERATIONS;
            else {
                MI_TRY(pg_linearise(c, d, cur));       // (its cost is F_new's bits again: the same arithmetic in the same order)
                linearisations++;
                final_is_candidate = false;
                MI_TRY(clock.mark(3));
            }
        } else {
            rejections++;
            if (rejections >= PG_MAX_REJECTIONS) stop = MI_STOP_ERROR_INCREASED;
            else lambda *= 10.0;
        }
    }

    // nothing has been written to a caller's array so far
    MI_HIP(hipMemcpyAsync(poses12.data(), cur, sizeof(double) * PG_POSE * Vn, hipMemcpyDeviceToHost, c->stream));
    if (out_weights) MI_HIP(hipMemcpyAsync(out_weights, final_is_candidate ? b.w_c.p : b.w.p, sizeof(double) * (size_t)E, hipMemcpyDeviceToHost, c->stream));
    if (out_chi2) MI_HIP(hipMemcpyAsync(out_chi2, final_is_candidate ? b.chi2_c.p : b.chi2.p, sizeof(double) * (size_t)E, hipMemcpyDeviceToHost, c->stream));
    MI_HIP(hipStreamSynchronize(c->stream));
    if (out_poses != poses) std::memmove(out_poses, poses, sizeof(double) * 16 * Vn);
    for (size_t k = 0; k < Vn; k++)
        for (int i = 0; i < 3; i++) {
            for (int j = 0; j < 3; j++) out_poses[16 * k + 4 * j + i] = poses12[PG_POSE * k + 3 * i + j];
            out_poses[16 * k + 12 + i] = poses12[PG_POSE * k + 9 + i];
        }
    report[1] = F; report[2] = linearisations; report[3] = accepted; report[4] = (double)pcg_total; report[5] = lambda; report[6] = stop; report[7] = last_rel;
    for (int i = 0; i < 8; i++) out_report[i] = report[i];
    MI_TRY(clock.mark(6));
    clock.finish();
    return MI_OK;
}

extern "C" int mi_pose_graph_system(mi_ctx* c, const double* poses, int V, const int* edge_source, const int* edge_target, const double* edge_T,
                                    const double* edge_information, const unsigned char* edge_uncertain, int E, const mi_pose_graph_params* params,
                                    const double* p_in, int solve, double* out_r, double* out_chi2, double* out_w, double* out_M, double* out_h,
                                    double* out_diag, double* out_g, double* out_Hp, double* out_x, double* out_pcg, double* out_cost)
{
    const char* who = "mi_pose_graph_system";
    const PgInputs in{poses, V, edge_source, edge_target, edge_T, edge_information, edge_uncertain, E, params};
    MI_TRY(pg_check_scalars(who, c, in));
    if (p_in)
        for (size_t i = 0; i < 6 * (size_t)V; i++)
            if (!std::isfinite(p_in[i])) { set_error("%s: p[%zu] has a non-finite entry", who, i / 6); return MI_ERR_INVALID_ARG; }
    std::vector<double> poses12, Z, L;
    std::vector<int> long_nodes;
    MI_TRY(pg_check_and_pack(who, in, poses12, Z, L, long_nodes));
    if (c->distributed()) { set_error("%s: single-GPU contexts only", who); return MI_ERR_STATE; }
    MI_ENTER(c);
    mi_ctx::PoseGraphBuffers& b = c->pose_graph;
    StageClock clock(c, b.ms);
    const size_t Vn = (size_t)V, En = (size_t)E;

    if (E == 0) {                      // no edge: every per-node result is 0
        if (out_diag) std::memset(out_diag, 0, sizeof(double) * PG_TRI * Vn);
        for (double* o : {out_g, out_Hp, out_x})
            if (o) std::memset(o, 0, sizeof(double) * 6 * Vn);
        if (out_pcg) { out_pcg[0] = 0.0; out_pcg[1] = 0.0; }
        if (out_cost) *out_cost = 0.0;
        clock.finish();
        return MI_OK;
    }

    CallBuffers bufs;
    PgDevice d;
    MI_TRY(pg_setup(c, clock, bufs, in, poses12, Z, L, long_nodes, p_in != nullptr, &d));
    const double lambda = params->lambda0;
    PgState h{};
    MI_TRY(pg_linearise(c, d, b.poses.p));
    MI_TRY(clock.mark(3));
    if (p_in) {
        std::vector<double> p_soa(6 * Vn);
        for (size_t k = 0; k < Vn; k++)
            for (int i = 0; i < 6; i++) p_soa[(size_t)i * Vn + k] = (int)k == params->reference_node ? 0.0 : p_in[6 * k + i];
        MI_TRY(host_to_device(c, b.user_p.p, p_soa.data(), sizeof(double) * 6 * Vn));
        MI_HIP(pg_product(d.g, d.t, b.diag.p, lambda, b.user_p.p, b.hp.p, b.pq_node.p, b.parts.p, nullptr, c->stream));
    }
    if (solve) MI_TRY(pg_solve(c, who, d, lambda, *params, &h));
    else MI_TRY(pg_read_state(c, &h));
    MI_TRY(clock.mark(4));

    std::vector<double> r, M, hh, diag, grad, hp, x;
    if (out_r) MI_TRY(pg_download_soa(c, b.r.p, En, 6, r));
    if (out_M) MI_TRY(pg_download_soa(c, b.M.p, En, PG_TRI, M));
    if (out_h) MI_TRY(pg_download_soa(c, b.h.p, En, 6, hh));
    if (out_diag) MI_TRY(pg_download_soa(c, b.diag.p, Vn, PG_TRI, diag));
    if (out_g) MI_TRY(pg_download_soa(c, b.grad.p, Vn, 6, grad));
    if (out_Hp && p_in) MI_TRY(pg_download_soa(c, b.hp.p, Vn, 6, hp));
    if (out_x && solve) MI_TRY(pg_download_soa(c, b.x.p, Vn, 6, x));
    if (out_chi2) MI_HIP(hipMemcpyAsync(out_chi2, b.chi2.p, sizeof(double) * En, hipMemcpyDeviceToHost, c->stream));
    if (out_w) MI_HIP(hipMemcpyAsync(out_w, b.w.p, sizeof(double) * En, hipMemcpyDeviceToHost, c->stream));
    MI_HIP(hipStreamSynchronize(c->stream));
    if (out_r) pg_transpose_out(r, En, 6, out_r);
    if (out_M) pg_transpose_out(M, En, PG_TRI, out_M);
    if (out_h) pg_transpose_out(hh, En, 6, out_h);
    if (out_diag) pg_transpose_out(diag, Vn, PG_TRI, out_diag);
    if (out_g) pg_transpose_out(grad, Vn, 6, out_g);
    if (out_Hp && p_in) pg_transpose_out(hp, Vn, 6, out_Hp);
    if (out_x && solve) pg_transpose_out(x, Vn, 6, out_x);
    if (out_pcg && solve) { out_pcg[0] = (double)h.iterations; out_pcg[1] = h.gg > 0.0 ? std::sqrt(h.rr) / std::sqrt(h.gg) : 0.0; }
    if (out_cost) *out_cost = h.cost[0];
    MI_TRY(clock.mark(6));
    clock.finish();
    return MI_OK;
}

extern "C" int mi_pose_graph_times(mi_ctx* c, double out_ms[MI_POSE_GRAPH_STAGES])
{
    return stage_times("mi_pose_graph_times", c ? c->pose_graph.ms : nullptr, out_ms);
}
