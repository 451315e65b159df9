// The arithmetic between a point and its bin of a Scan Context descriptor (mi_scan_context, mi_slam.h), stated once for the device kernel
// (scan_context_kernels.hip), the host tables (mi_scan_context_tables) and the CPU self-test (tests/scan_context_bin_selftest.cpp, which
// includes this header alone, without HIP).  Everything is fp64, every operation rounded once and none fused (both builds use
// -ffp-contract=off); no transcendental function and no square root stands between a point and its bin: the ring comes from comparisons
// against the squared ring edges, the sector from sign tests against the boundary directions.
#pragma once

#if defined(__HIPCC__)
#define MISLAM_SC_HD __host__ __device__
#else
#define MISLAM_SC_HD
#endif

namespace mislam {

constexpr int SC_MAX_RINGS = 32;         // MI_SCAN_CONTEXT_MAX_RINGS
constexpr int SC_MAX_SECTORS = 64;       // MI_SCAN_CONTEXT_MAX_SECTORS
constexpr float SC_MAX_ABS = 1e18f;      // a coordinate above this is refused: (2e18)^2 + (2e18)^2 is far inside fp64

// The ring of a squared planar distance: the number of inner edges ring_edge2[1 .. rings - 1] at or below d2, so an exact edge belongs to
// the ring outside it; -1 at or beyond ring_edge2[rings] = max_radius^2 (and for a NaN, which the callers have refused before).
MISLAM_SC_HD inline int sc_ring(double d2, const double* ring_edge2, int rings)
{
    if (!(d2 < ring_edge2[rings])) return -1;
    int r = 0;
    for (int e = 1; e < rings; e++) r += ring_edge2[e] <= d2 ? 1 : 0;
    return r;
}

// The sector of an offset (dx, dy) from the centre.  sector_dir[2 j], sector_dir[2 j + 1] = (c_j, s_j), the direction of the boundary at
// which sector j begins, at the angle 2 pi j / sectors; boundaries j with 2 j < sectors lie in the upper half-plane [0, pi), the others in
// the lower one [pi, 2 pi).  The half-plane first: upper for dy > 0, or dy == 0 and dx > 0; lower for dy < 0, or dy == 0 and dx < 0; the
// point exactly at the centre goes to sector 0.  Then the number of boundaries of the point's own half-plane that it has passed: boundary
// j is passed when c_j dy - s_j dx >= 0 -- two products and one difference -- so a point exactly on a boundary belongs to the sector that
// begins there.  The sector is the last boundary of the half-plane below (or, with none passed, of the other half-plane) plus that number.
MISLAM_SC_HD inline int sc_sector(double dx, double dy, const double* sector_dir, int sectors)
{
    const bool upper = dy > 0.0 || (dy == 0.0 && dx > 0.0);
    const bool lower = dy < 0.0 || (dy == 0.0 && dx < 0.0);
    if (!upper && !lower) return 0;
    const int first_lower = (sectors + 1) / 2;                       // the lowest j with 2 j >= sectors
    const int j0 = upper ? 0 : first_lower, j1 = upper ? first_lower : sectors;
    int passed = 0;
    for (int j = j0; j < j1; j++) {
        const double a = sector_dir[2 * j] * dy, b = sector_dir[2 * j + 1] * dx;
        passed += (a - b) >= 0.0 ? 1 : 0;
    }
    const int s = j0 - 1 + passed;                                   // upper: boundary 0 is always passed (1 * dy - 0 * dx >= 0)
    return s < 0 ? 0 : s;                                            // (does not happen; keeps every index in range whatever the table holds)
}

}  // namespace mislam
