// Stand-alone check of the CPD drivers' host plan (cuda-slam_amd/csrc/cpd_plan.hpp): the header alone, no HIP.  (a) literal expectations that pin
// the rounding rules of the route decision, the weight clamp and the two "how often" rules; (b) one line per case of the chunk plans, the FGT's
// constants and the monomial tables, which tests/test_cpd_plan.py compares with the Python restatements the float64 tests rest on.  That test
// builds this file plain and under the address and undefined-behaviour sanitizers and runs both.
#include "../cuda-slam_amd/csrc/cpd_plan.hpp"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

using namespace mislam;

static int g_failed = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); g_failed++; } } while (0)

static unsigned bits(float f) { unsigned u; memcpy(&u, &f, sizeof u); return u; }

int main()
{
    {   // "full": always the FGT; sigma^2 below the DOUBLE 0.05 is replaced by (float)0.05 -- and (double)0.05f lies above the double 0.05
        CHECK((double)0.05f > 0.05);
        CpdRouteChoice r = cpd_route(MI_CPD_APPROX_FULL, 0.05f, 1.0f);
        CHECK(r.route == CpdRoute::Fgt && !r.clamped && bits(r.sigma2) == bits(0.05f));
        const float below = nextafterf(0.05f, 0.f);
        r = cpd_route(MI_CPD_APPROX_FULL, below, 1.0f);
        CHECK(r.route == CpdRoute::Fgt && r.clamped && bits(r.sigma2) == bits((float)0.05) && bits(r.sigma2) != bits(below));
        r = cpd_route(MI_CPD_APPROX_FULL, 2.0f, 1.0f);
        CHECK(r.route == CpdRoute::Fgt && !r.clamped && r.sigma2 == 2.0f);
        r = cpd_route(MI_CPD_APPROX_FULL, 1e-6f, 50.0f);
        CHECK(r.route == CpdRoute::Fgt && r.clamped && bits(r.sigma2) == bits(0.05f));
    }
    for (const float s0 : {1.0f, 37.5f}) {   // "hybrid": the FGT iff (double)sigma2 > 0.015 * (double)sigma2_init, at the float on each side
        const double thr = 0.015 * (double)s0;
        float lo = (float)thr, hi;
        if ((double)lo > thr) { hi = lo; lo = nextafterf(hi, 0.f); } else hi = nextafterf(lo, INFINITY);
        CHECK((double)lo <= thr && (double)hi > thr && nextafterf(lo, INFINITY) == hi);
        CpdRouteChoice r = cpd_route(MI_CPD_APPROX_HYBRID, hi, s0);
        CHECK(r.route == CpdRoute::Fgt && !r.clamped && bits(r.sigma2) == bits(hi));
        r = cpd_route(MI_CPD_APPROX_HYBRID, lo, s0);
        CHECK(r.route == CpdRoute::Truncated && !r.clamped && bits(r.sigma2) == bits(lo));
        r = cpd_route(MI_CPD_APPROX_HYBRID, 0.01f, s0);                       // (hybrid never clamps, however small)
        CHECK(r.route == CpdRoute::Truncated && !r.clamped && r.sigma2 == 0.01f);
    }
    {   // at sigma2_init = 1 the float 0.015f itself lies BELOW the double product 0.015 * 1.0: a float comparison would call it equal
        CHECK((double)0.015f < 0.015 && cpd_route(MI_CPD_APPROX_HYBRID, 0.015f, 1.0f).route == CpdRoute::Truncated);
        CHECK(cpd_route(MI_CPD_APPROX_NONE, 0.f, 0.f).route == CpdRoute::Exact && !cpd_route(MI_CPD_APPROX_NONE, 1e-9f, 1.f).clamped);
    }
    {   // the weight clamp (coherentpointdrift.cpp:93-96): at and beyond 0 and 1, and nothing in between
        CHECK(bits(cpd_clamp_weight(0.0f)) == bits(1e-6f) && bits(cpd_clamp_weight(-1.0f)) == bits(1e-6f) && bits(cpd_clamp_weight(-0.0f)) == bits(1e-6f));
        CHECK(bits(cpd_clamp_weight(1.0f)) == bits(1.0f - 1e-6f) && bits(cpd_clamp_weight(2.0f)) == bits(1.0f - 1e-6f));
        const float tiny = nextafterf(0.f, 1.f), almost = nextafterf(1.f, 0.f);
        CHECK(bits(cpd_clamp_weight(tiny)) == bits(tiny) && bits(cpd_clamp_weight(almost)) == bits(almost) && cpd_clamp_weight(0.3f) == 0.3f);
    }
    const int sizes[] = {1, 2, 63, 64, 65, 2047, 2048, 2049, 4096, 100000, 1000000};
    {   // the sync_every estimate stays in [1, 8]: 8 where an iteration is all gaps, 1 where one iteration outlasts the budget
        for (int m : sizes)
            for (int n : sizes)
                for (int ranks : {1, 2, 8}) { const int b = cpd_sync_every_estimate(m, n, ranks); CHECK(b >= 1 && b <= 8); }
        CHECK(cpd_sync_every_estimate(1, 1, 1) == 8 && cpd_sync_every_estimate(2048, 2048, 1) == 8);
        CHECK(cpd_sync_every_estimate(1000000, 1000000, 1) == 1 && cpd_sync_every_estimate(2147483647, 2147483647, 8) == 1);
        CHECK(cpd_sync_every_estimate(35947, 35947, 1) == 1 && cpd_sync_every_estimate(35947, 35947, 8) == 6);
    }
    {   // the batched call's iterations per launch stay in [4, 64]
        const long long pairs[] = {1, 1LL << 20, 1LL << 24, 1LL << 26, 1LL << 31};
        const int want[] = {64, 64, 4, 4, 4};
        for (int i = 0; i < 5; i++) { const int it = cpd_batch_iters(pairs[i]); CHECK(it >= 4 && it <= 64 && it == want[i]); }
        CHECK(cpd_batch_iters(0) == 64 && cpd_batch_iters(1LL << 22) == 16);
    }
    {   // rows of M-step partial sums: 64 points a row behind the E-step's own kernels, 256 behind the stand-alone ones, a tile a row behind K7t
        CHECK(cpd_sum_blocks(1) == 1 && cpd_sum_blocks(64) == 1 && cpd_sum_blocks(65) == 2 && cpd_sum_blocks(32768) == 512 && cpd_sum_blocks(1000000) == 512);
        CHECK(cpd_standalone_sum_blocks(1) == 1 && cpd_standalone_sum_blocks(256) == 1 && cpd_standalone_sum_blocks(257) == 2 &&
              cpd_standalone_sum_blocks(131072) == 512 && cpd_standalone_sum_blocks(1000000) == 512);
        CHECK(cpd_trunc_tiles(1) == 1 && cpd_trunc_tiles(64) == 1 && cpd_trunc_tiles(65) == 2);
        CHECK(cpd_trunc_rows(0, 2) == 2 && cpd_trunc_rows(3, 3) == 1 && cpd_trunc_rows(0, 4096) == 4096 && cpd_trunc_rows(10, 5000) == 4096);
    }
    // ---- (b) the lines tests/test_cpd_plan.py reads
    for (int cu : {1, 256, 304})
        for (int m : sizes)
            for (int n : sizes) {
                const CpdChunkPlan p = cpd_chunk_plan(cu, m, n);
                CHECK(p.k_chunks >= 1 && p.k_chunks <= PLAN_CPD_MAX_CHUNKS && p.x_chunks >= 1 && p.x_chunks <= PLAN_CPD_MAX_CHUNKS);
                CHECK(p.k_chunk_len % PLAN_CPD_T == 0 && (long long)p.k_chunks * p.k_chunk_len >= m && (long long)(p.k_chunks - 1) * p.k_chunk_len < m);
                CHECK(p.x_chunk_len % PLAN_CPD_T == 0 && (long long)p.x_chunks * p.x_chunk_len >= n && (long long)(p.x_chunks - 1) * p.x_chunk_len < n);
                printf("chunks %d %d %d %d %d %d %d %d %d\n", cu, m, n, p.k_chunks, p.k_chunk_len, p.x_chunks, p.x_chunk_len, cpd_trunc_tiles(m), cpd_trunc_tiles(n));
            }
    const int fgt_sizes[][2] = {{2, 2}, {400, 500}, {700, 300}, {35947, 35947}};
    const float weights[] = {1e-6f, 0.3f, 1.0f - 1e-6f};
    for (const auto& mn : fgt_sizes)
        for (const float s2 : {2.0f, 0.3f, 0.05f, 1e-4f})
            for (const float s0 : {1.0f, 50.0f}) {
                const int K = fgt_cluster_count(mn[0], mn[1], s2, s0);
                CHECK(K >= 1 && K <= std::min(mn[0], mn[1]));
                printf("cells %d %d %08x %08x %d %08x\n", mn[0], mn[1], bits(s2), bits(s0), K, bits(fgt_hsigma(s2)));
                for (const float wt : weights) printf("ndi %d %d %08x %08x %08x\n", mn[0], mn[1], bits(s2), bits(wt), bits(fgt_ndi(s2, wt, mn[0], mn[1])));
            }
    for (int p : {1, 2, 8, 16}) {
        std::vector<unsigned int> mono; std::vector<float> ck; std::vector<int> hpos;
        fgt_build_tables(p, mono, ck, hpos);
        CHECK((int)mono.size() == fgt_pd(p) && ck.size() == mono.size() && hpos.size() == mono.size());
        printf("pd %d %d\n", p, fgt_pd(p));
        for (size_t t = 0; t < mono.size(); t++) printf("table %d %zu %u %08x %d\n", p, t, mono[t], bits(ck[t]), hpos[t]);
    }
    if (g_failed) { printf("%d checks FAILED\n", g_failed); return 1; }
    printf("cpd plan selftest ok\n");
    return 0;
}
