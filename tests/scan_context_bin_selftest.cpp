// Host self-test of cuda-slam_amd/csrc/scan_context_bin.hpp, the arithmetic between a point and its bin of mi_scan_context: the header alone,
// no HIP.  Built and run by tests/test_scan_context_bin.py, plain and under the address and undefined-behaviour sanitizers.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../cuda-slam_amd/csrc/scan_context_bin.hpp"

using namespace mislam;

static int failures = 0;
#define EXPECT(cond)                                                     \
    do {                                                                 \
        if (!(cond)) {                                                   \
            std::printf("line %d: %s\n", __LINE__, #cond);               \
            failures++;                                                  \
        }                                                                \
    } while (0)

// the tables as the library's host function states them
static void tables(int rings, int sectors, double max_radius, std::vector<double>& edge2, std::vector<double>& dir)
{
    edge2.assign(rings + 1, 0.0);
    dir.assign(2 * sectors, 0.0);
    for (int r = 0; r < rings; r++) {
        const double e = (max_radius * r) / rings;
        edge2[r] = e * e;
    }
    edge2[rings] = max_radius * max_radius;
    static const double axis[4][2] = {{1, 0}, {0, 1}, {-1, 0}, {0, -1}};
    for (int j = 0; j < sectors; j++) {
        if ((4 * j) % sectors == 0) {
            dir[2 * j] = axis[4 * j / sectors][0];
            dir[2 * j + 1] = axis[4 * j / sectors][1];
        } else if (sectors % 2 == 0 && j >= sectors / 2) {
            dir[2 * j] = -dir[2 * (j - sectors / 2)];
            dir[2 * j + 1] = -dir[2 * (j - sectors / 2) + 1];
        } else {
            const double ang = (2.0 * M_PI * j) / sectors;
            dir[2 * j] = std::cos(ang);
            dir[2 * j + 1] = std::sin(ang);
        }
    }
}

static unsigned long long state = 88172645463325252ull;
static double uniform()
{
    state ^= state << 13; state ^= state >> 7; state ^= state << 17;
    return (double)(state >> 11) / 9007199254740992.0;
}

int main()
{
    const int shapes[][2] = {{20, 60}, {1, 1}, {32, 64}, {7, 13}, {4, 8}, {3, 2}, {5, 3}};
    for (const auto& shape : shapes) {
        const int rings = shape[0], sectors = shape[1];
        std::vector<double> edge2, dir;
        tables(rings, sectors, 80.0, edge2, dir);

        // rings: an exact edge belongs to the ring outside it, max_radius^2 and beyond to none, a NaN to none
        for (int r = 0; r < rings; r++) {
            EXPECT(sc_ring(edge2[r], edge2.data(), rings) == r);
            EXPECT(sc_ring(std::nextafter(edge2[r + 1], 0.0), edge2.data(), rings) == r);
        }
        EXPECT(sc_ring(edge2[rings], edge2.data(), rings) == -1);
        EXPECT(sc_ring(1e300, edge2.data(), rings) == -1);
        EXPECT(sc_ring(std::nan(""), edge2.data(), rings) == -1);

        // sectors: the centre, both signs of zero; a point exactly on a boundary direction belongs to the sector that begins there
        EXPECT(sc_sector(0.0, 0.0, dir.data(), sectors) == 0);
        EXPECT(sc_sector(-0.0, -0.0, dir.data(), sectors) == 0);
        EXPECT(sc_sector(3.0, 0.0, dir.data(), sectors) == 0);
        EXPECT(sc_sector(3.0, -0.0, dir.data(), sectors) == 0);
        EXPECT(sc_sector(-3.0, 0.0, dir.data(), sectors) == sectors / 2);
        if (sectors % 4 == 0) {
            EXPECT(sc_sector(0.0, 5.0, dir.data(), sectors) == sectors / 4);
            EXPECT(sc_sector(0.0, -5.0, dir.data(), sectors) == 3 * sectors / 4);
        }
        for (int j = 0; j < sectors; j++) EXPECT(sc_sector(4.0 * dir[2 * j], 4.0 * dir[2 * j + 1], dir.data(), sectors) == j);      // a power of two scales exactly

        // random points away from the boundaries: the sector of the angle
        for (int i = 0; i < 20000; i++) {
            const double dx = 200.0 * uniform() - 100.0, dy = 200.0 * uniform() - 100.0;
            double w = std::atan2(dy, dx);
            if (w < 0) w += 2.0 * M_PI;
            const double u = w / (2.0 * M_PI) * sectors;
            if (std::fabs(u - std::nearbyint(u)) < 1e-9) continue;
            const int want = (int)std::floor(u) >= sectors ? sectors - 1 : (int)std::floor(u);
            EXPECT(sc_sector(dx, dy, dir.data(), sectors) == want);
            const double d2 = dx * dx + dy * dy, v = std::sqrt(d2) / 80.0 * rings;
            if (std::fabs(v - std::nearbyint(v)) < 1e-9) continue;
            EXPECT(sc_ring(d2, edge2.data(), rings) == (v >= rings ? -1 : (int)std::floor(v)));
        }

        // whatever a table holds, the indices stay in range
        std::vector<double> junk(2 * sectors);
        for (double& v : junk) v = 2.0 * uniform() - 1.0;
        for (int i = 0; i < 2000; i++) {
            const int s = sc_sector(2.0 * uniform() - 1.0, 2.0 * uniform() - 1.0, junk.data(), sectors);
            EXPECT(s >= 0 && s < sectors);
        }
    }
    if (failures) {
        std::printf("scan_context_bin selftest: %d failures\n", failures);
        return 1;
    }
    std::printf("scan_context_bin selftest ok\n");
    return 0;
}
