// The CPD drivers' host plan: everything they decide from sizes, sigma^2 and the parameters before anything is enqueued -- chunk plans, rows of
// partial sums, the FGT's cell count and constants, how often the host looks at the state, the route of an approximated E-step, the monomial
// tables.  Pure arithmetic: nothing from HIP, so tests/cpd_plan_selftest.cpp builds it with a host compiler alone and ties it to the Python
// restatements the float64 tests rest on (tests/estep_reference.py plan_chunks / plan, tests/fgt_reference.py cluster_count / ndi / pd_of).
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>

#include "../../include/mi_slam.h"

namespace mislam {

// The kernel headers' values (cpd_kernels.h, kernels.h: both need the HIP runtime), stated again for the plan; cpd_workspace.h, which sees
// both, ties each pair with a static_assert.
constexpr int PLAN_CPD_T = 8;                        // CPD_T
constexpr int PLAN_CPD_MAX_CHUNKS = 256;             // CPD_MAX_CHUNKS
constexpr int PLAN_CPD_TRUNC_TILE = 64;              // CPD_TRUNC_TILE
constexpr int PLAN_CPD_TRUNC_MAX_BLOCKS = 4096;      // CPD_TRUNC_MAX_BLOCKS
constexpr int PLAN_ICP_MAX_PARTIAL_BLOCKS = 512;     // ICP_MAX_PARTIAL_BLOCKS

// Chunk the broadcast axis so that the grid has >= ~8 workgroups per CU even for bunny-sized clouds.
static inline void plan_chunks(int cu_count, int owners, int owner_r, int stream_len, int* chunks, int* chunk_len)
{
    const int owner_blocks = std::max(1, (owners + 256 * owner_r - 1) / (256 * owner_r));
    int ch = (cu_count * 8 + owner_blocks - 1) / owner_blocks;
    ch = std::max(1, std::min(ch, std::min(PLAN_CPD_MAX_CHUNKS, std::max(1, stream_len / (PLAN_CPD_T * 8)))));
    *chunk_len = ((stream_len + ch - 1) / ch + PLAN_CPD_T - 1) / PLAN_CPD_T * PLAN_CPD_T;
    *chunks = (stream_len + *chunk_len - 1) / *chunk_len;
}
// K7a (owners: the n fixed points, four per lane; stream: the m moving points) and K7b (owners: the moving points, two per lane; stream: the fixed points)
struct CpdChunkPlan { int k_chunks, k_chunk_len, x_chunks, x_chunk_len; };
static inline CpdChunkPlan cpd_chunk_plan(int cu_count, int m, int n)
{
    CpdChunkPlan p{};
    plan_chunks(cu_count, n, 4, m, &p.k_chunks, &p.k_chunk_len);
    plan_chunks(cu_count, m, 2, n, &p.x_chunks, &p.x_chunk_len);
    return p;
}

// workgroups of the E-step's post kernels (a quad of lanes per point there: 64 points per workgroup) = rows of M-step partial sums they leave
static inline int cpd_sum_blocks(int n) { return std::max(1, std::min(PLAN_ICP_MAX_PARTIAL_BLOCKS, (n + 63) / 64)); }
// ... and of the STAND-ALONE sums kernels (cpd_xsums / cpd_ksums: one lane per point, 256 per workgroup).  ADVICE r04: launched with
// cpd_sum_blocks they left three quarters of their workgroups storing zeros below 32 768 points.  Their fp64 partials are grouped differently
// from the fused ones' (256 against 64 points per row) -- the same sums to ~1e-16 relative, not the same bits.
static inline int cpd_standalone_sum_blocks(int n) { return std::max(1, std::min(PLAN_ICP_MAX_PARTIAL_BLOCKS, (n + 255) / 256)); }

// K7t: tiles of a cloud along its curve, and the rows of M-step partial sums its two kernels leave for tiles [lo, hi)
static inline int cpd_trunc_tiles(int n) { return (n + PLAN_CPD_TRUNC_TILE - 1) / PLAN_CPD_TRUNC_TILE; }
static inline int cpd_trunc_rows(int tile_lo, int tile_hi) { return std::max(1, std::min(PLAN_CPD_TRUNC_MAX_BLOCKS, tile_hi - tile_lo)); }

// coherentpointdrift.cpp:93-96
static inline float cpd_clamp_weight(float weight)
{
    if (weight <= 0.0f) weight = 1e-6f;
    if (weight >= 1.0f) weight = 1.0f - 1e-6f;
    return weight;
}

// Iterations of the exact E-step between two host checks when the caller names none: enough that the check (a 160-byte read-back: ~35 us of
// idle device) stays a few per cent of them, few enough that what is enqueued past the stopping iteration (kernels that return at once,
// ~15 us per iteration) stays small: about a millisecond of E-steps.  From the GLOBAL sizes (every rank of a multi-GPU context picks the
// same batch): the two passes over the pair space run at ~2.5e12 pairs/s on one GPU, the small kernels and gaps take ~60 us per iteration.
// ranks: those that share the pair space (1 where every rank holds both clouds whole)
static inline int cpd_sync_every_estimate(int m, int n_total, int ranks)
{
    const double pairs = (double)m * (double)n_total;
    const double est_s = 2.0 * pairs / 2.5e12 / (double)ranks + 6e-5;
    return std::max(1, std::min(8, (int)(1.2e-3 / est_s)));
}

// The batched call: a launch ends after this many EM iterations of its longest problem: two passes over at most 2^26 pairs per workgroup and
// launch (~10 ms on one CU), never fewer than 4 iterations (a launch boundary is a host round trip)
static inline int cpd_batch_iters(long long max_pairs) { return (int)std::max(4LL, std::min(64LL, (1LL << 26) / std::max(1LL, max_pairs))); }

// The E-step of one iteration of a registration.  ComputePMatrixFast, coherentpointdrift.cpp:141-167: the comparisons are double there
// (0.05 and 0.015 are doubles).  "full": always the FGT, sigma^2 held at 0.05 from below (clamped: the state block's value is to be
// replaced by .sigma2); "hybrid": the FGT while sigma^2 > 0.015 sigma^2_0, the truncated exact E-step from there on.
enum class CpdRoute { Exact, Fgt, Truncated };
struct CpdRouteChoice { CpdRoute route; float sigma2; bool clamped; };
static inline CpdRouteChoice cpd_route(int approximation, float sigma2, float sigma2_init)
{
    if (approximation == MI_CPD_APPROX_NONE) return {CpdRoute::Exact, sigma2, false};
    if (approximation == MI_CPD_APPROX_FULL) {
        if ((double)sigma2 < 0.05) return {CpdRoute::Fgt, (float)0.05, true};
        return {CpdRoute::Fgt, sigma2, false};
    }
    return {(double)sigma2 > 0.015 * (double)sigma2_init ? CpdRoute::Fgt : CpdRoute::Truncated, sigma2, false};
}

// ---- Fast Gauss Transform (ComputePMatrixWithFGT, common/cpdutils.cpp:19-77)
// K of the transform: cpdutils.cpp:36
static inline int fgt_cluster_count(int m, int n, float sigma2, float sigma2_init)
{
    return (int)std::round(std::min({(float)n, (float)m, 50.0f + sigma2_init / sigma2}));
}
// ndi: cpdutils.cpp:45 -- pow and the numerator in double, the denominator a float product, narrowed to float
static inline float fgt_ndi(float sigma2, float weight, int m, int n)
{
    return (float)((std::pow(2 * 3.14159265358979323846 * sigma2, (double)(3.f * 0.5f)) * weight * m) / (double)((1 - weight) * n));
}
static inline float fgt_hsigma(float sigma2) { return std::sqrt(2.0f * sigma2); }       // cpdutils.cpp:31
static inline int fgt_pd(int p) { return p * (p + 1) * (p + 2) / 6; }                     // nchoosek(p + 2, 3), fgt.cpp:69

// The monomial tables of truncation order p (FgtTables, cpd_fgt.h): exponents a | b << 8 | c << 16, C_k, Horner slot
static inline void fgt_build_tables(int p, std::vector<unsigned int>& mono, std::vector<float>& ck, std::vector<int>& hpos)
{
    const int pd = fgt_pd(p);
    mono.assign(pd, 0u); ck.assign(pd, 0.f); hpos.assign(pd, 0);
    // slot of exponents (a, b, c) in the reference's graded order: all of degree d-1 first, then x-power descending, then y-power
    auto slot = [](int a, int b, int c) { const int d = a + b + c, r = d - a; return d * (d + 1) * (d + 2) / 6 + r * (r + 1) / 2 + (r - b); };
    for (int d = 0; d < p; d++)
        for (int a = d; a >= 0; a--)
            for (int b = d - a; b >= 0; b--) {
                const int c = d - a - b, t = slot(a, b, c);
                mono[t] = (unsigned)a | ((unsigned)b << 8) | ((unsigned)c << 16);
                // 2^|alpha| / alpha!, rounded the way ComputeC_k walks the recursion: z steps, then y steps, then x steps, each step
                // C = float(2.0 * C) followed by C = float(C / (double)q), q = the running exponent (fgt.cpp:236-238)
                float C = 1.0f;
                const int steps[3] = {c, b, a};
                for (int axis = 0; axis < 3; axis++)
                    for (int q = 1; q <= steps[axis]; q++) { C = (float)(2.0 * C); C = (float)(C / (double)q); }
                ck[t] = C;
            }
    int h = 0;                                                     // Horner traversal of fgt_predict_kernel
    for (int a = p - 1; a >= 0; a--)
        for (int b = p - 1 - a; b >= 0; b--)
            for (int c = p - 1 - a - b; c >= 0; c--) hpos[slot(a, b, c)] = h++;
}

}  // namespace mislam
