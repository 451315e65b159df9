// K56-K63: pose-graph optimisation (mi_pose_graph_optimize, mi_pose_graph_system; driver: pose_graph_api.hip).  The edge's arithmetic is
// pose_graph_terms.hpp's, the 6 x 6 solve of the preconditioner and the pose update are plane_solve.hpp's, the sums over nodes and edges
// are reduce.hpp's.  No floating-point atomics: every sum has a fixed order that depends on the graph's shape alone (kernels.h states the
// rule of a node's list), so the same input gives the same bits.
//   K56  incidence lists: the (node, 2 * edge + side) pairs for the library's radix sort, and the CSR offsets by binary search
//   K57  edge terms: one lane per edge -- r, chi2, w, and with the system asked for M (21) and h (6); the cost's partial sums
//   K58  cost finish: one workgroup adds the partial sums into the state block
//   K59  node gather: a node's diagonal block (21) and gradient (6) over its list
//   K60  product: q = (H + lambda diag H) p over the same lists, fused with the partial sums of p . q
//   K61  vector kernels of the inner solve: begin (r = -g, z, p), update (x, r, z and the partial sums of r . z and r . r), direction (p)
//   K62  scalar kernels: one workgroup turns partial sums into alpha, beta, the residual norm, the count and the done flag
//   K63  apply: candidate poses exp(x_k) T_k
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "plane_solve.hpp"
#include "pose_graph_terms.hpp"
#include "reduce.hpp"

namespace mislam {

// ---- K56
__device__ __forceinline__ int pg_entry_node(const int* __restrict__ src, const int* __restrict__ tgt, int entry)
{
    return (entry & 1) ? tgt[entry >> 1] : src[entry >> 1];
}

// keys[i] = (the node of entry vals_in[i], or of entry i where vals_in is null) >> shift; vals_out[i] = i where vals_in is null
__global__ __launch_bounds__(256) void pg_incidence_keys_kernel(const int* __restrict__ src, const int* __restrict__ tgt, const int* __restrict__ vals_in,
                                                                int n2, int shift, unsigned int* __restrict__ keys, int* __restrict__ vals_out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n2) return;
    const int entry = vals_in ? vals_in[i] : i;
    keys[i] = (unsigned int)pg_entry_node(src, tgt, entry) >> shift;
    if (!vals_in) vals_out[i] = i;
}

hipError_t pg_incidence_keys(const int* src, const int* tgt, const int* vals_in, int n2, int shift, unsigned int* keys, int* vals_out, hipStream_t s)
{
    if (n2 <= 0) return hipSuccess;
    hipLaunchKernelGGL(pg_incidence_keys_kernel, dim3(pg_blocks(n2)), dim3(256), 0, s, src, tgt, vals_in, n2, shift, keys, vals_out);
    return hipGetLastError();
}

// offsets[k] = the number of list entries whose node is below k, k in [0, V]
__global__ __launch_bounds__(256) void pg_offsets_kernel(PgGraph g, int* __restrict__ offsets)
{
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    if (k > (long long)g.V) return;
    int lo = 0, hi = 2 * g.E;
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if ((long long)pg_entry_node(g.src, g.tgt, g.list[mid]) < k) lo = mid + 1; else hi = mid;
    }
    offsets[k] = lo;
}

hipError_t pg_build_offsets(const PgGraph& g, int* offsets, hipStream_t s)
{
    const unsigned int blocks = (unsigned int)(((long long)g.V + 1 + 255) / 256);
    hipLaunchKernelGGL(pg_offsets_kernel, dim3(blocks), dim3(256), 0, s, g, offsets);
    return hipGetLastError();
}

// ---- K57
__global__ __launch_bounds__(256) void pg_edge_kernel(PgGraph g, const double* __restrict__ poses, PgTerms t, int system, double* __restrict__ cost_parts)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    const size_t E = (size_t)g.E;
    double acc[1] = {0.0};
    if (e < g.E) {
        const int a = g.src[e], b = g.tgt[e];
        double Ts[PG_POSE], Tt[PG_POSE], Z[PG_POSE], L[PG_TRI];
#pragma unroll
        for (int i = 0; i < PG_POSE; i++) {
            Ts[i] = poses[(size_t)a * PG_POSE + i];
            Tt[i] = poses[(size_t)b * PG_POSE + i];
            Z[i] = g.Z[(size_t)i * E + e];
        }
#pragma unroll
        for (int i = 0; i < PG_TRI; i++) L[i] = g.L[(size_t)i * E + e];
        const bool uncertain = g.uncertain != nullptr && g.uncertain[e] != 0;
        double r[6], chi2, w, share, M[PG_TRI], h[6];
        if (system) {
            pg_edge_terms(Ts, Tt, Z, L, uncertain, g.mu, true, r, &chi2, &w, &share, M, h);
#pragma unroll
            for (int i = 0; i < 6; i++) { t.r[(size_t)i * E + e] = r[i]; t.h[(size_t)i * E + e] = h[i]; }
#pragma unroll
            for (int i = 0; i < PG_TRI; i++) t.M[(size_t)i * E + e] = M[i];
        } else {
            pg_edge_terms(Ts, Tt, Z, L, uncertain, g.mu, false, r, &chi2, &w, &share, M, h);
        }
        t.chi2[e] = chi2;
        t.w[e] = w;
        acc[0] = share;
    }
    block_sum_store<1>(acc, cost_parts + blockIdx.x);
}

hipError_t pg_edge_terms_launch(const PgGraph& g, const double* poses, const PgTerms& t, int system, double* cost_parts, hipStream_t s)
{
    if (g.E <= 0) return hipSuccess;
    hipLaunchKernelGGL(pg_edge_kernel, dim3(pg_blocks(g.E)), dim3(256), 0, s, g, poses, t, system, cost_parts);
    return hipGetLastError();
}

// ---- K58
__global__ __launch_bounds__(256) void pg_cost_finish_kernel(const double* __restrict__ parts, int nparts, PgState* __restrict__ st, int slot)
{
    __shared__ double lds[256];
    double out[1];
    reduce_partials<1>(parts, nparts, out, lds);
    if (threadIdx.x == 0) st->cost[slot] = out[0];
}

hipError_t pg_cost_finish(const double* cost_parts, int nparts, PgState* st, int slot, hipStream_t s)
{
    hipLaunchKernelGGL(pg_cost_finish_kernel, dim3(1), dim3(256), 0, s, cost_parts, nparts, st, slot);
    return hipGetLastError();
}

// ---- the sums over a node's list (the rule: kernels.h)
// one lane alone, for a list of at most PG_LONG_LIST entries: the list's own order
template <int N, class Term>
__device__ __forceinline__ void pg_list_sum_lane(const int* __restrict__ list, int lo, int hi, Term&& term, double (&acc)[N])
{
#pragma unroll
    for (int c = 0; c < N; c++) acc[c] = 0.0;
    for (int i = lo; i < hi; i++) {
        double v[N];
        term(list[i], v);
#pragma unroll
        for (int c = 0; c < N; c++) acc[c] += v[c];
    }
}
// one wave (a workgroup of 64 lanes): strided partial sums, then lane c adds component c's 64 partial sums from lane 0 on.  lds: 64 * (N | 1)
// doubles; every lane leaves with the sums.
template <int N, class Term>
__device__ __forceinline__ void pg_list_sum_wave(const int* __restrict__ list, int lo, int hi, Term&& term, double* lds, double (&acc)[N])
{
    constexpr int S = N | 1;
    const int lane = threadIdx.x;
    double part[N];
#pragma unroll
    for (int c = 0; c < N; c++) part[c] = 0.0;
    for (int i = lo + lane; i < hi; i += 64) {
        double v[N];
        term(list[i], v);
#pragma unroll
        for (int c = 0; c < N; c++) part[c] += v[c];
    }
#pragma unroll
    for (int c = 0; c < N; c++) lds[lane * S + c] = part[c];
    __syncthreads();
    double sum = 0.0;
    if (lane < N)
        for (int l = 0; l < 64; l++) sum += lds[l * S + lane];
    __syncthreads();
    if (lane < N) lds[lane] = sum;
    __syncthreads();
#pragma unroll
    for (int c = 0; c < N; c++) acc[c] = lds[c];
    __syncthreads();
}

// ---- K59
struct PgGatherTerm {
    const double* M; const double* h; size_t E;
    __device__ __forceinline__ void operator()(int entry, double (&v)[27]) const
    {
        const int e = entry >> 1;
        const double sign = (entry & 1) ? -1.0 : 1.0;         // g_s += h, g_t -= h; the diagonal block takes M on both sides
#pragma unroll
        for (int c = 0; c < PG_TRI; c++) v[c] = M[(size_t)c * E + e];
#pragma unroll
        for (int c = 0; c < 6; c++) v[PG_TRI + c] = sign * h[(size_t)c * E + e];
    }
};
__device__ __forceinline__ void pg_gather_store(const double (&acc)[27], int k, size_t V, double* __restrict__ diag, double* __restrict__ grad)
{
#pragma unroll
    for (int c = 0; c < PG_TRI; c++) diag[(size_t)c * V + k] = acc[c];
#pragma unroll
    for (int c = 0; c < 6; c++) grad[(size_t)c * V + k] = acc[PG_TRI + c];
}

__global__ __launch_bounds__(256) void pg_gather_kernel(PgGraph g, PgTerms t, double* __restrict__ diag, double* __restrict__ grad)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= g.V) return;
    const int lo = g.offsets[k], hi = g.offsets[k + 1];
    if (hi - lo > PG_LONG_LIST) return;                       // the wave kernel's
    double acc[27];
    pg_list_sum_lane<27>(g.list, lo, hi, PgGatherTerm{t.M, t.h, (size_t)g.E}, acc);
    pg_gather_store(acc, k, (size_t)g.V, diag, grad);
}

__global__ __launch_bounds__(64) void pg_gather_long_kernel(PgGraph g, PgTerms t, double* __restrict__ diag, double* __restrict__ grad)
{
    __shared__ double lds[64 * 27];
    const int k = g.long_nodes[blockIdx.x];
    double acc[27];
    pg_list_sum_wave<27>(g.list, g.offsets[k], g.offsets[k + 1], PgGatherTerm{t.M, t.h, (size_t)g.E}, lds, acc);
    if (threadIdx.x == 0) pg_gather_store(acc, k, (size_t)g.V, diag, grad);
}

hipError_t pg_node_gather(const PgGraph& g, const PgTerms& t, double* diag, double* grad, hipStream_t s)
{
    if (g.n_long > 0) hipLaunchKernelGGL(pg_gather_long_kernel, dim3(g.n_long), dim3(64), 0, s, g, t, diag, grad);
    hipLaunchKernelGGL(pg_gather_kernel, dim3(pg_blocks(g.V)), dim3(256), 0, s, g, t, diag, grad);
    return hipGetLastError();
}

// ---- K60
struct PgProductTerm {
    const double* M; const double* p; const int* src; const int* tgt; size_t E, V;
    __device__ __forceinline__ void operator()(int entry, double (&v)[6]) const
    {
        const int e = entry >> 1;
        const int a = src[e], b = tgt[e];
        double M21[PG_TRI], d[6], y[6];
#pragma unroll
        for (int c = 0; c < PG_TRI; c++) M21[c] = M[(size_t)c * E + e];
#pragma unroll
        for (int c = 0; c < 6; c++) d[c] = p[(size_t)c * V + a] - p[(size_t)c * V + b];
        pg_sym_apply(M21, d, y);
        const double sign = (entry & 1) ? -1.0 : 1.0;         // (H p)_s += M (p_s - p_t), (H p)_t -= M (p_s - p_t)
#pragma unroll
        for (int c = 0; c < 6; c++) v[c] = sign * y[c];
    }
};
// the damping, the store and p_k . q_k of node k; the reference node's row is 0
__device__ __forceinline__ double pg_product_finish(const PgGraph& g, const double (&acc)[6], int k, const double* __restrict__ diag, double lambda,
                                                    const double* __restrict__ p, double* __restrict__ q)
{
    const size_t V = (size_t)g.V;
    double dot = 0.0;
#pragma unroll
    for (int c = 0; c < 6; c++) {
        const double pc = p[(size_t)c * V + k];
        double qc = acc[c] + (lambda * diag[(size_t)pg_tri_diag(c) * V + k]) * pc;
        if (k == g.reference) qc = 0.0;
        q[(size_t)c * V + k] = qc;
        dot += pc * qc;
    }
    return dot;
}

__global__ __launch_bounds__(64) void pg_product_long_kernel(PgGraph g, PgTerms t, const double* __restrict__ diag, double lambda, const double* __restrict__ p,
                                                             double* __restrict__ q, double* __restrict__ pq_node, const PgState* __restrict__ st)
{
    __shared__ double lds[64 * 7];
    if (st && st->done != 0) return;
    const int k = g.long_nodes[blockIdx.x];
    double acc[6];
    pg_list_sum_wave<6>(g.list, g.offsets[k], g.offsets[k + 1], PgProductTerm{t.M, p, g.src, g.tgt, (size_t)g.E, (size_t)g.V}, lds, acc);
    if (threadIdx.x == 0) pq_node[k] = pg_product_finish(g, acc, k, diag, lambda, p, q);
}

__global__ __launch_bounds__(256) void pg_product_kernel(PgGraph g, PgTerms t, const double* __restrict__ diag, double lambda, const double* __restrict__ p,
                                                         double* __restrict__ q, const double* __restrict__ pq_node, double* __restrict__ parts,
                                                         const PgState* __restrict__ st)
{
    if (st && st->done != 0) return;
    const int k = blockIdx.x * 256 + threadIdx.x;
    double dot[2] = {0.0, 0.0};
    if (k < g.V) {
        const int lo = g.offsets[k], hi = g.offsets[k + 1];
        if (hi - lo > PG_LONG_LIST) {
            dot[0] = pq_node[k];                              // the wave kernel ran in front of this one
        } else {
            double acc[6];
            pg_list_sum_lane<6>(g.list, lo, hi, PgProductTerm{t.M, p, g.src, g.tgt, (size_t)g.E, (size_t)g.V}, acc);
            dot[0] = pg_product_finish(g, acc, k, diag, lambda, p, q);
        }
    }
    block_sum_store<2>(dot, parts + 2 * (size_t)blockIdx.x);
}

hipError_t pg_product(const PgGraph& g, const PgTerms& t, const double* diag, double lambda, const double* p, double* q, double* pq_node, double* parts,
                      const PgState* st, hipStream_t s)
{
    if (g.n_long > 0) hipLaunchKernelGGL(pg_product_long_kernel, dim3(g.n_long), dim3(64), 0, s, g, t, diag, lambda, p, q, pq_node, st);
    hipLaunchKernelGGL(pg_product_kernel, dim3(pg_blocks(g.V)), dim3(256), 0, s, g, t, diag, lambda, p, q, pq_node, parts, st);
    return hipGetLastError();
}

// ---- K61
// z = (D_k + lambda diag D_k)^-1 r by plane_solve6's scaled LDL^T, afresh at every use (no inverse is stored); a block it calls degenerate
// -- a node without edges has D_k = 0 -- is preconditioned by the identity
__device__ __forceinline__ void pg_precondition(const double* __restrict__ diag, double lambda, int k, size_t V, const double (&r)[6], double (&z)[6])
{
    double D[PG_TRI], neg[6];
#pragma unroll
    for (int c = 0; c < PG_TRI; c++) D[c] = diag[(size_t)c * V + k];
#pragma unroll
    for (int c = 0; c < 6; c++) { D[pg_tri_diag(c)] = D[pg_tri_diag(c)] + lambda * D[pg_tri_diag(c)]; neg[c] = -r[c]; }
    if (!plane_solve6(D, neg, z, nullptr)) {
#pragma unroll
        for (int c = 0; c < 6; c++) z[c] = r[c];
    }
}

__global__ __launch_bounds__(256) void pg_pcg_begin_kernel(PgGraph g, const double* __restrict__ diag, const double* __restrict__ grad, double lambda, PgVectors v)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    const size_t V = (size_t)g.V;
    double dots[2] = {0.0, 0.0};
    if (k < g.V) {
        double r[6], z[6];
#pragma unroll
        for (int c = 0; c < 6; c++) r[c] = k == g.reference ? 0.0 : -grad[c * V + k];
        pg_precondition(diag, lambda, k, V, r, z);
#pragma unroll
        for (int c = 0; c < 6; c++) {
            v.x[c * V + k] = 0.0; v.r[c * V + k] = r[c]; v.z[c * V + k] = z[c]; v.p[c * V + k] = z[c];
            dots[0] += r[c] * z[c];
            dots[1] += r[c] * r[c];
        }
    }
    block_sum_store<2>(dots, v.parts + 2 * (size_t)blockIdx.x);
}

__global__ __launch_bounds__(256) void pg_pcg_update_kernel(PgGraph g, const double* __restrict__ diag, double lambda, PgVectors v, const PgState* __restrict__ st)
{
    if (st->done != 0) return;
    const int k = blockIdx.x * 256 + threadIdx.x;
    const size_t V = (size_t)g.V;
    const double alpha = st->alpha;
    double dots[2] = {0.0, 0.0};
    if (k < g.V) {
        double r[6], z[6];
#pragma unroll
        for (int c = 0; c < 6; c++) {
            v.x[c * V + k] = v.x[c * V + k] + alpha * v.p[c * V + k];
            r[c] = v.r[c * V + k] - alpha * v.q[c * V + k];
        }
        pg_precondition(diag, lambda, k, V, r, z);
#pragma unroll
        for (int c = 0; c < 6; c++) {
            v.r[c * V + k] = r[c]; v.z[c * V + k] = z[c];
            dots[0] += r[c] * z[c];
            dots[1] += r[c] * r[c];
        }
    }
    block_sum_store<2>(dots, v.parts + 2 * (size_t)blockIdx.x);
}

__global__ __launch_bounds__(256) void pg_pcg_direction_kernel(int V, PgVectors v, const PgState* __restrict__ st)
{
    if (st->done != 0) return;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= 6 * (size_t)V) return;
    v.p[i] = v.z[i] + st->beta * v.p[i];
}

// ---- K62: mode 0 behind begin, 1 behind the product (alpha), 2 behind the update (beta, the stop rule)
__global__ __launch_bounds__(256) void pg_pcg_scalar_kernel(const double* __restrict__ parts, int nparts, PgState* __restrict__ st, int mode, double tolerance,
                                                            int max_iterations)
{
    __shared__ double lds[256];
    if (mode != 0 && st->done != 0) return;
    double out[2];
    reduce_partials<2>(parts, nparts, out, lds);
    if (threadIdx.x != 0) return;
    if (mode == 0) {
        st->rz = out[0]; st->gg = out[1]; st->rr = out[1];
        st->pq = 0.0; st->alpha = 0.0; st->beta = 0.0;
        st->tolerance = tolerance; st->max_iterations = max_iterations; st->iterations = 0; st->breakdown = 0;
        st->done = (!(out[1] > 0.0) || max_iterations <= 0 || sqrt(out[1]) <= tolerance * sqrt(out[1])) ? 1 : 0;
    } else if (mode == 1) {
        st->pq = out[0];
        if (!(out[0] > 0.0) || !(out[0] <= 1.7976931348623157e308)) { st->done = 1; st->breakdown = 1; }   // the step so far stands
        else st->alpha = st->rz / out[0];
    } else {
        st->beta = out[0] / st->rz;
        st->rz = out[0]; st->rr = out[1];
        st->iterations = st->iterations + 1;
        if (!(sqrt(out[1]) > st->tolerance * sqrt(st->gg)) || st->iterations >= st->max_iterations) st->done = 1;
        if (!(out[0] > 0.0)) st->done = 1;                     // r . z = 0: nothing left to divide by
    }
}

hipError_t pg_pcg_begin(const PgGraph& g, const double* diag, const double* grad, double lambda, double tolerance, int max_iterations, const PgVectors& v,
                        PgState* st, hipStream_t s)
{
    const int nb = pg_blocks(g.V);
    hipLaunchKernelGGL(pg_pcg_begin_kernel, dim3(nb), dim3(256), 0, s, g, diag, grad, lambda, v);
    hipLaunchKernelGGL(pg_pcg_scalar_kernel, dim3(1), dim3(256), 0, s, v.parts, nb, st, 0, tolerance, max_iterations);
    return hipGetLastError();
}

hipError_t pg_pcg_iterations(const PgGraph& g, const PgTerms& t, const double* diag, double lambda, const PgVectors& v, PgState* st, int count, hipStream_t s)
{
    const int nb = pg_blocks(g.V);
    const unsigned int vb = (unsigned int)((6 * (size_t)g.V + 255) / 256);
    for (int i = 0; i < count; i++) {
        hipError_t e = pg_product(g, t, diag, lambda, v.p, v.q, v.pq_node, v.parts, st, s);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(pg_pcg_scalar_kernel, dim3(1), dim3(256), 0, s, v.parts, nb, st, 1, 0.0, 0);
        hipLaunchKernelGGL(pg_pcg_update_kernel, dim3(nb), dim3(256), 0, s, g, diag, lambda, v, st);
        hipLaunchKernelGGL(pg_pcg_scalar_kernel, dim3(1), dim3(256), 0, s, v.parts, nb, st, 2, 0.0, 0);
        hipLaunchKernelGGL(pg_pcg_direction_kernel, dim3(vb), dim3(256), 0, s, g.V, v, st);
    }
    return hipGetLastError();
}

// ---- K63
__global__ __launch_bounds__(256) void pg_apply_kernel(PgGraph g, const double* __restrict__ poses, const double* __restrict__ x, double* __restrict__ out)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= g.V) return;
    const size_t V = (size_t)g.V;
    double d[6], R[9], t[3];
    bool moves = k != g.reference && g.offsets[k + 1] > g.offsets[k];
    bool any = false;
#pragma unroll
    for (int c = 0; c < 6; c++) { d[c] = x[c * V + k]; any = any || d[c] != 0.0; }
#pragma unroll
    for (int i = 0; i < 9; i++) R[i] = poses[(size_t)k * PG_POSE + i];
#pragma unroll
    for (int i = 0; i < 3; i++) t[i] = poses[(size_t)k * PG_POSE + 9 + i];
    if (moves && any) {                                        // a node that does not move keeps its pose's bits
        const double w[3] = {d[0], d[1], d[2]}, vv[3] = {d[3], d[4], d[5]}, c0[3] = {0.0, 0.0, 0.0};
        double dR[9];
        plane_rodrigues(w, dR);
        plane_compose(dR, vv, c0, R, t);
    }
#pragma unroll
    for (int i = 0; i < 9; i++) out[(size_t)k * PG_POSE + i] = R[i];
#pragma unroll
    for (int i = 0; i < 3; i++) out[(size_t)k * PG_POSE + 9 + i] = t[i];
}

hipError_t pg_apply_step(const PgGraph& g, const double* poses, const double* x, double* out_poses, hipStream_t s)
{
    hipLaunchKernelGGL(pg_apply_kernel, dim3(pg_blocks(g.V)), dim3(256), 0, s, g, poses, x, out_poses);
    return hipGetLastError();
}

// loads this translation unit's code object at mi_ctx_preload (kernels.h)
__global__ void preload_pose_graph_kernels_kernel() {}
hipError_t preload_pose_graph_kernels()
{
    hipFuncAttributes attr;
    return hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(preload_pose_graph_kernels_kernel));
}

}  // namespace mislam
