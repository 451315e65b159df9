// Host self-test of cuda-slam_amd/csrc/tsdf_ray.hpp, the arithmetic of mi_tsdf_integrate and mi_tsdf_extract: this file includes the header
// alone (no HIP) and is built as a program of its own, plain and under the address and undefined-behaviour sanitizers
// (tests/test_tsdf_ray.py), with -ffp-contract=off as the library is.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../cuda-slam_amd/csrc/tsdf_ray.hpp"

using namespace mislam;

static int failures = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); failures++; } \
    } while (0)

struct Sample { int k, c[3]; double f; };

static std::vector<Sample> walk(const float* T, const float p[3], float voxel, float tau, const float origin[3], float lo = 0.f, float hi = INFINITY, bool* ok = nullptr)
{
    std::vector<Sample> out;
    float w[3], o[3];
    tsdf_move(T, p[0], p[1], p[2], w, o);
    TsdfRay r;
    if (!tsdf_ray(w, o, lo, hi, &r)) { if (ok) *ok = true; return out; }
    const bool fine = tsdf_walk(r, (int)tsdf_half_steps(voxel, tau), voxel, origin, tau, [&](int k, const int c[3], double f) { out.push_back({k, {c[0], c[1], c[2]}, f}); });
    if (ok) *ok = fine;
    return out;
}

int main()
{
    const float zero[3] = {0.f, 0.f, 0.f};
    CHECK(tsdf_half_steps(0.1f, 0.3f) == 6.0 && tsdf_half_steps(1.f, 0.5f) == 1.0 && tsdf_half_steps(0.5f, 4.f) == 16.0 && tsdf_half_steps(0.5f, 4.25f) == 17.0);

    // the move: the identity through the arithmetic, and a column-major pose
    {
        float w[3], o[3];
        tsdf_move(nullptr, 1.5f, -2.f, 0.25f, w, o);
        CHECK(w[0] == 1.5f && w[1] == -2.f && w[2] == 0.25f && o[0] == 0.f && o[1] == 0.f && o[2] == 0.f);
        const float T[16] = {0.f, 1.f, 0.f, 0.f, -1.f, 0.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 10.f, 20.f, 30.f, 1.f};      // a quarter turn about z, then (10, 20, 30)
        tsdf_move(T, 1.f, 2.f, 3.f, w, o);
        CHECK(w[0] == 8.f && w[1] == 21.f && w[2] == 33.f && o[0] == 10.f && o[1] == 20.f && o[2] == 30.f);
    }

    // a ray along x through voxel centres, voxel 1, tau 1: samples at 3.5, 4, .. 5.5 on lattice planes and centres; a sample exactly on a
    // plane belongs to the voxel above; every voxel once
    {
        const float T[16] = {1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.5f, 0.5f, 1.f};       // the sensor at (0, 0.5, 0.5)
        const float p[3] = {4.5f, 0.f, 0.f};
        const std::vector<Sample> s = walk(T, p, 1.f, 1.f, zero);
        CHECK(s.size() == 3);
        if (s.size() == 3) {
            CHECK(s[0].k == -2 && s[0].c[0] == 3 && s[0].f == 1.0);
            CHECK(s[1].k == -1 && s[1].c[0] == 4 && s[1].f == 0.0);
            CHECK(s[2].k == 1 && s[2].c[0] == 5 && s[2].f == -1.0);                 // sdf == -tau exactly: kept
            for (const Sample& e : s) CHECK(e.c[1] == 0 && e.c[2] == 0);
        }
        // tau a little shorter: S stays 1 (floor(0.99 / 0.5)), samples at 4, 4.5, 5; the voxel behind has sdf = -1 < -tau: dropped
        const std::vector<Sample> t = walk(T, p, 1.f, 0.99f, zero);
        CHECK(t.size() == 1 && t[0].k == -1 && t[0].c[0] == 4 && t[0].f == 0.0);
    }

    // a ray lying in the lattice plane z = 1: its samples belong to the voxels above the plane
    {
        const float T[16] = {1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.5f, 0.5f, 1.f, 1.f};      // the sensor at (0.5, 0.5, 1)
        const float q[3] = {2.f, 0.f, 0.f};
        const std::vector<Sample> s = walk(T, q, 1.f, 1.f, zero);
        CHECK(s.size() == 3);
        for (const Sample& e : s) CHECK(e.c[2] == 1 && e.c[1] == 0);
        if (s.size() == 3) CHECK(s[0].c[0] == 1 && s[0].f == 1.0 && s[1].c[0] == 2 && s[1].f == 0.0 && s[2].c[0] == 3 && s[2].f == -1.0);
    }

    // a ray shorter than the band: the samples at s_k <= 0 do not exist (k = -2: s = 0 exactly; k = -3: negative)
    {
        const float p[3] = {0.25f, 0.f, 0.f};
        const float origin[3] = {-8.f, -8.f, -8.f};
        const std::vector<Sample> s = walk(nullptr, p, 0.25f, 0.5f, origin);
        CHECK(!s.empty() && s[0].k == -1);
        for (const Sample& e : s) CHECK(e.k >= -1 && e.c[0] >= 32);
    }

    // the gates: rho == 0, below min_range, above max_range, exactly on either gate
    {
        bool ok = false;
        const float at[3] = {0.f, 0.f, 0.f}, p[3] = {3.f, 0.f, 4.f};
        CHECK(walk(nullptr, at, 1.f, 1.f, zero, 0.f, INFINITY, &ok).empty() && ok);
        CHECK(walk(nullptr, p, 1.f, 1.f, zero, 5.5f, INFINITY).empty() && walk(nullptr, p, 1.f, 1.f, zero, 0.f, 4.5f).empty());
        CHECK(!walk(nullptr, p, 1.f, 1.f, zero, 5.f, 5.f + 1.f).empty() && !walk(nullptr, p, 1.f, 1.f, zero, 0.f, 5.f).empty());
        const float huge[3] = {1e18f, 0.f, 0.f};
        CHECK(walk(nullptr, huge, 1e-3f, 1e-3f, zero, 0.f, INFINITY, &ok).empty() && !ok);             // a voxel coordinate out of range: refused
    }

    // the crossing and its corner cases
    {
        double r = -7.0;
        CHECK(tsdf_crossing(0.5, -0.5, &r) && r == 0.5 && tsdf_crossing(-0.25, 0.75, &r) && r == 0.25);
        CHECK(tsdf_crossing(0.0, 0.5, &r) && r == 0.0 && std::signbit(r));                              // f0 == 0, f1 > 0: at the centre itself
        CHECK(tsdf_crossing_coord(5, 0.f, 0.5f, r) == 2.75f);
        r = -7.0;
        CHECK(!tsdf_crossing(0.0, 0.0, &r) && !tsdf_crossing(-0.0, 0.0, &r) && r == -7.0);            // f0 == f1 == 0: none, and no 0 / 0
        CHECK(!tsdf_crossing(1.0, -1.0, &r) && !tsdf_crossing(0.5, 0.25, &r) && !tsdf_crossing(-0.5, 0.0, &r));
        CHECK(tsdf_crossing(1.0, -0.5, &r) && tsdf_crossing(0.5, 0.0, &r) && r == 1.0);
        CHECK(tsdf_crossing_coord(5, 0.f, 0.5f, 0.5) == 3.f && tsdf_crossing_coord(-1, 1.f, 0.5f, 1.0) == 1.25f);
    }

    // the gradient's three cases, and none
    CHECK(tsdf_gradient(true, -0.5, 0.125, true, 0.75) == 0.625);
    CHECK(tsdf_gradient(false, 99.0, 0.125, true, 0.75) == 0.625 && tsdf_gradient(true, -0.5, 0.125, false, 99.0) == 0.625);
    CHECK(tsdf_gradient(false, 99.0, 0.125, false, 99.0) == 0.0);

    // the normal: unit length, a zero vector stays zero
    {
        const double gi[3] = {3.0, 0.0, 4.0}, gj[3] = {3.0, 0.0, 4.0}, none[3] = {0.0, 0.0, 0.0}, back[3] = {-3.0, 0.0, -4.0};
        float n[3];
        tsdf_normal(gi, gj, 0.25, n);
        CHECK(n[0] == 0.6f && n[1] == 0.f && n[2] == 0.8f);
        tsdf_normal(none, none, 0.5, n);
        CHECK(n[0] == 0.f && n[1] == 0.f && n[2] == 0.f);
        tsdf_normal(gi, back, 0.5, n);
        CHECK(n[0] == 0.f && n[1] == 0.f && n[2] == 0.f);
    }

    // the map's checks name the lowest refused row
    {
        const int coord[12] = {0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1};
        float tsdf[4] = {0.f, 1.f, -1.f, 0.5f}, weight[4] = {1.f, 2.f, 3.f, 4.f};
        int row = -1, lo[3], hi[3];
        CHECK(tsdf_check_map(coord, tsdf, weight, 4, &row, lo, hi) == TSDF_MAP_OK && lo[0] == 0 && hi[0] == 1 && hi[1] == 1 && hi[2] == 1);
        CHECK(tsdf_check_map(nullptr, nullptr, nullptr, 0, &row, lo, hi) == TSDF_MAP_OK);
        const int swapped[12] = {0, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0, 1}, twice[6] = {3, 3, 3, 3, 3, 3}, wide[3] = {1 << 30, 0, 0};
        CHECK(tsdf_check_map(swapped, tsdf, weight, 4, &row, lo, hi) == TSDF_MAP_ORDER && row == 2);
        CHECK(tsdf_check_map(twice, tsdf, weight, 2, &row, lo, hi) == TSDF_MAP_ORDER && row == 1);
        CHECK(tsdf_check_map(wide, tsdf, weight, 1, &row, lo, hi) == TSDF_MAP_COORD && row == 0);
        weight[2] = 0.f;
        CHECK(tsdf_check_map(coord, tsdf, weight, 4, &row, lo, hi) == TSDF_MAP_WEIGHT && row == 2);
        weight[2] = INFINITY; weight[3] = NAN;
        CHECK(tsdf_check_map(coord, tsdf, weight, 4, &row, lo, hi) == TSDF_MAP_WEIGHT && row == 2);
        weight[2] = 3.f; weight[3] = 4.f; tsdf[1] = 1.0000001f;
        CHECK(tsdf_check_map(coord, tsdf, weight, 4, &row, lo, hi) == TSDF_MAP_VALUE && row == 1);
        tsdf[1] = NAN;
        CHECK(tsdf_check_map(coord, tsdf, weight, 4, &row, lo, hi) == TSDF_MAP_VALUE && row == 1);
    }

    if (failures) { std::printf("tsdf_ray selftest: %d failures\n", failures); return 1; }
    std::printf("tsdf_ray selftest ok\n");
    return 0;
}
