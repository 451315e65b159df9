// Host self-test of cuda-slam_amd/csrc/tsdf_cast.hpp, the arithmetic of mi_tsdf_raycast: this file includes the header (and through it
// tsdf_ray.hpp) alone, no HIP, and is built as a program of its own, plain and under the address and undefined-behaviour sanitizers
// (tests/test_tsdf_cast.py), with -ffp-contract=off as the library is.  Without arguments it checks a few facts with known answers.  With
// `in out` it reads a small map, a pose and rays from `in` (the layout below, written by the test), casts every ray twice -- every sample
// visited, and with empty-space skipping over a host set of marked blocks -- and writes per ray the direction, where the march ended, r, the
// depth, point and normal, and the voxel of every sample to `out`, for the test to compare with tests/tsdf_raycast_reference.py bit for bit.
#include <array>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <vector>

#include "../cuda-slam_amd/csrc/tsdf_cast.hpp"

using namespace mislam;

static int failures = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); failures++; } \
    } while (0)

struct Header {
    int32_t nv, n, has_pose, skip_forced;        // skip_forced 1: skip whatever tsdf_cast_skip_sound says (never set by the test for a comparison)
    float origin[3], voxel, min_weight, min_range, max_range, pad;
    float T[16];
};
struct Record {
    double d[3], r;
    int32_t end_k, trilinear, hit, same_with_skip;
    float depth, xyz[3], normal[3], pad;
};

template <class T>
static bool read_all(std::FILE* f, std::vector<T>& v) { return v.empty() || std::fread(v.data(), sizeof(T), v.size(), f) == v.size(); }

static bool same_bits(const TsdfCastHit& a, const TsdfCastHit& b)
{
    auto bits = [](float x) { uint32_t u; std::memcpy(&u, &x, 4); return u; };
    bool ok = bits(a.depth) == bits(b.depth) && a.k == b.k && a.trilinear == b.trilinear && a.r == b.r;
    for (int i = 0; i < 3; i++) ok = ok && bits(a.xyz[i]) == bits(b.xyz[i]) && bits(a.normal[i]) == bits(b.normal[i]);
    return ok;
}

static int run_file(const char* in, const char* out)
{
    std::FILE* f = std::fopen(in, "rb");
    if (!f) { std::printf("cannot open %s\n", in); return 2; }
    Header h;
    if (std::fread(&h, sizeof h, 1, f) != 1 || h.nv < 0 || h.n < 1) { std::printf("bad header\n"); return 2; }
    std::vector<int32_t> coord(3 * (size_t)h.nv);
    std::vector<float> tsdf((size_t)h.nv), weight((size_t)h.nv), dirs(3 * (size_t)h.n);
    if (!read_all(f, coord) || !read_all(f, tsdf) || !read_all(f, weight) || !read_all(f, dirs)) { std::printf("short file\n"); return 2; }
    std::fclose(f);

    int row = 0, cmin[3], cmax[3];
    if (tsdf_check_map(coord.data(), tsdf.data(), weight.data(), h.nv, &row, cmin, cmax) != TSDF_MAP_OK) { std::printf("map refused at row %d\n", row); return 2; }
    std::map<std::array<int, 3>, int> rows;
    std::set<std::array<int, 3>> marked;
    for (int i = 0; i < h.nv; i++) {
        if (!(weight[i] >= h.min_weight)) continue;
        const int* c = &coord[3 * (size_t)i];
        rows[{c[0], c[1], c[2]}] = i;
        for (int dz = -1; dz <= 1; dz++)
            for (int dy = -1; dy <= 1; dy++)
                for (int dx = -1; dx <= 1; dx++) marked.insert({(c[0] >> TSDF_SKIP_SHIFT) + dx, (c[1] >> TSDF_SKIP_SHIFT) + dy, (c[2] >> TSDF_SKIP_SHIFT) + dz});
    }
    auto lookup = [&](int cx, int cy, int cz) { auto it = rows.find({cx, cy, cz}); return it == rows.end() ? -1 : it->second; };
    long long asked = 0;
    auto occupied = [&](int bx, int by, int bz) { asked++; return marked.count({bx, by, bz}) != 0; };

    TsdfCastGeom g;
    for (int a = 0; a < 3; a++) g.origin[a] = h.origin[a];
    g.voxel = h.voxel; g.min_range = h.min_range;
    const double steps = tsdf_cast_steps(h.voxel, h.min_range, h.max_range);
    if (!(steps >= 1.0 && steps <= (double)TSDF_RAYCAST_MAX_STEPS)) { std::printf("K = %g\n", steps); return 2; }
    g.steps = (int)steps;
    const float* T = h.has_pose ? h.T : nullptr;
    const bool skip = h.skip_forced != 0 || tsdf_cast_skip_sound(T, h.origin, h.voxel, h.max_range);

    std::FILE* o = std::fopen(out, "wb");
    if (!o) { std::printf("cannot open %s\n", out); return 2; }
    const int32_t head[4] = {g.steps, skip ? 1 : 0, 0, 0};
    std::fwrite(head, sizeof head, 1, o);
    std::vector<int32_t> voxels(4 * (size_t)g.steps);
    for (int i = 0; i < h.n; i++) {
        Record rec{};
        TsdfCastRay ray{};
        TsdfCastHit plain{}, skipped{};
        std::fill(voxels.begin(), voxels.end(), 0);
        if (tsdf_cast_dir(T, dirs[3 * (size_t)i], dirs[3 * (size_t)i + 1], dirs[3 * (size_t)i + 2], &ray)) {
            const bool hit = tsdf_cast(ray, g, tsdf.data(), lookup, false, occupied, &plain);
            const bool hit2 = tsdf_cast(ray, g, tsdf.data(), lookup, skip, occupied, &skipped);
            // the samples a sound skip leaves out are unobserved, and those neither end a march nor stand before a hit: the same end, the same bits
            rec.same_with_skip = hit == hit2 && same_bits(plain, skipped);
            rec.hit = hit;
            for (int a = 0; a < 3; a++) { rec.d[a] = ray.d[a]; rec.xyz[a] = plain.xyz[a]; rec.normal[a] = plain.normal[a]; }
            rec.r = plain.r; rec.end_k = plain.k; rec.trilinear = plain.trilinear; rec.depth = plain.depth;
            for (int k = 0; k < g.steps; k++) {
                int c[3] = {0, 0, 0};
                voxels[4 * (size_t)k] = tsdf_cast_sample_voxel(ray, g, k, c) ? 1 : 0;
                for (int a = 0; a < 3; a++) voxels[4 * (size_t)k + 1 + a] = voxels[4 * (size_t)k] ? c[a] : 0;
            }
        } else {
            rec.same_with_skip = 1;
            rec.end_k = g.steps;
        }
        std::fwrite(&rec, sizeof rec, 1, o);
        std::fwrite(voxels.data(), sizeof(int32_t), voxels.size(), o);
    }
    std::fclose(o);
    std::printf("tsdf_cast selftest: %d rays, K = %d, skip %d, %lld block look-ups\n", h.n, g.steps, skip ? 1 : 0, asked);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 3) return run_file(argv[1], argv[2]);
    static_assert(sizeof(Header) == 4 * 4 + 8 * 4 + 16 * 4 && sizeof(Record) == 4 * 8 + 4 * 4 + 8 * 4, "the test reads and writes these layouts");

    // K: floor((max - min) / h) + 1 (the float 0.1 is a little above 0.1: 4 / 0.05 falls just short of 80)
    CHECK(tsdf_cast_steps(0.1f, 0.f, 4.f) == 80.0 && tsdf_cast_steps(0.125f, 0.f, 4.f) == 65.0 && tsdf_cast_steps(1.f, 0.f, 0.25f) == 1.0 && tsdf_cast_steps(1.f, 2.f, 3.f) == 3.0);
    CHECK(tsdf_cast_steps(1e-3f, 0.f, 1e3f) > (double)TSDF_RAYCAST_MAX_STEPS);

    // the skip's condition: (3 max|o| + 2 max|origin| + 3 max_range) / voxel <= 2^21
    {
        const float zero[3] = {0.f, 0.f, 0.f}, far[3] = {3e4f, 0.f, 0.f}, farther[3] = {2e6f, 0.f, 0.f};
        float T[16] = {1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f};
        CHECK(tsdf_cast_skip_sound(nullptr, zero, 0.1f, 4.f) && tsdf_cast_skip_sound(T, zero, 0.1f, 4.f));
        T[12] = 3e4f;
        CHECK(tsdf_cast_skip_sound(T, far, 0.1f, 4.f));                 // 1.5e6 + 120 <= 2^21
        T[12] = -2e6f;
        CHECK(!tsdf_cast_skip_sound(T, farther, 0.1f, 4.f) && !tsdf_cast_skip_sound(T, zero, 0.1f, 4.f) && !tsdf_cast_skip_sound(nullptr, farther, 0.1f, 4.f));
        CHECK(!tsdf_cast_skip_sound(nullptr, zero, 1e-3f, 1e3f));
    }

    // the direction: the identity through the arithmetic, a quarter turn, any length, no length
    {
        TsdfCastRay r;
        CHECK(tsdf_cast_dir(nullptr, 0.f, 3.f, 4.f, &r) && r.d[0] == 0.0 && r.d[1] == 0.6 && r.d[2] == 0.8 && r.o[0] == 0.0);
        const float T[16] = {0.f, 1.f, 0.f, 0.f, -1.f, 0.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 10.f, 20.f, 30.f, 1.f};
        CHECK(tsdf_cast_dir(T, 2.f, 0.f, 0.f, &r) && r.d[0] == 0.0 && r.d[1] == 1.0 && r.d[2] == 0.0 && r.o[0] == 10.0 && r.o[1] == 20.0 && r.o[2] == 30.0);
        CHECK(!tsdf_cast_dir(nullptr, 0.f, 0.f, 0.f, &r) && !tsdf_cast_dir(nullptr, -0.f, 0.f, 0.f, &r));
        CHECK(tsdf_cast_dir(nullptr, 1e18f, 1e18f, 1e18f, &r) && tsdf_cast_dir(nullptr, 1e-45f, 0.f, 0.f, &r) && r.d[0] == 1.0);
        const float big[16] = {3e38f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f};
        CHECK(!tsdf_cast_dir(big, 1e18f, 0.f, 0.f, &r));               // the fp32 product overflows: not finite, a miss
    }

    // two voxels along x, 0.5 and -0.5, voxel 1, seen from x = 0 along +x through their centres: samples at 0, 0.5, .. ; the sample at
    // 1.0 is the first in voxel 1 (a position on a lattice plane belongs to the voxel above), value 0.5; the sample at 2.0 is the first in
    // voxel 2, value -0.5: k = 4, a = 1.5, no trilinear field (corners missing), r = 0.5, depth 1.75, normal (-1, 0, 0)
    {
        const float tsdf[2] = {0.5f, -0.5f};
        auto lookup = [](int cx, int cy, int cz) { return cy == 0 && cz == 0 && (cx == 1 || cx == 2) ? cx - 1 : -1; };
        auto never = [](int, int, int) { return true; };
        TsdfCastGeom g = {{0.f, 0.f, 0.f}, 1.f, 0.f, 9};
        TsdfCastRay r = {{0.0, 0.5, 0.5}, {1.0, 0.0, 0.0}};
        TsdfCastHit hit;
        CHECK(tsdf_cast(r, g, tsdf, lookup, false, never, &hit) && hit.k == 4 && hit.trilinear == 0 && hit.r == 0.5 && hit.depth == 1.75f);
        CHECK(hit.xyz[0] == 1.75f && hit.xyz[1] == 0.5f && hit.xyz[2] == 0.5f && hit.normal[0] == -1.f && hit.normal[1] == 0.f && hit.normal[2] == 0.f);
        // from the other side the negative voxel comes first: a miss, ended at its first sample; from inside it too
        TsdfCastRay back = {{4.0, 0.5, 0.5}, {-1.0, 0.0, 0.0}}, inside = {{2.5, 0.5, 0.5}, {1.0, 0.0, 0.0}};
        CHECK(!tsdf_cast(back, g, tsdf, lookup, false, never, &hit) && hit.k == 3 && hit.depth == 0.f && hit.normal[0] == 0.f);
        CHECK(!tsdf_cast(inside, g, tsdf, lookup, false, never, &hit) && hit.k == 0);
        // too few samples to reach the surface: the march runs out
        g.steps = 4;
        CHECK(!tsdf_cast(r, g, tsdf, lookup, false, never, &hit) && hit.k == 4 && hit.depth == 0.f);
        // a gap between the positive and the negative voxel: positive -> unobserved -> negative is a miss
        auto gap = [](int cx, int cy, int cz) { return cy == 0 && cz == 0 ? (cx == 1 ? 0 : (cx == 3 ? 1 : -1)) : -1; };
        g.steps = 9;
        CHECK(!tsdf_cast(r, g, tsdf, gap, false, never, &hit) && hit.k == 6);
    }

    if (failures) { std::printf("tsdf_cast selftest: %d failures\n", failures); return 1; }
    std::printf("tsdf_cast selftest ok\n");
    return 0;
}
