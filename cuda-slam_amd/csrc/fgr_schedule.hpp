// The scale and the annealing schedule of mi_fgr_register (rule 3 of its contract in mi_slam.h), stated once for the device (the step and
// weights kernels of fgr_kernels.hip) and for the host (final_mu and the bounding boxes' diagonal in fgr_api.hip), and the host's reading of
// "the last linearisation" out of a finished loop.  Everything is fp64, one rounding per operation; nothing of HIP is needed, so
// tests/fgr_schedule_selftest.cpp compiles this header alone with a host compiler.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MISLAM_FGR_HD __host__ __device__
#else
#define MISLAM_FGR_HD
#endif

namespace mislam {

// the squared diagonal of a bounding box given as fp32 bounds: the extents subtracted in fp64, then ((dx dx + dy dy) + dz dz)
MISLAM_FGR_HD inline double fgr_diagonal2(const float lo[3], const float hi[3])
{
    const double dx = (double)hi[0] - (double)lo[0], dy = (double)hi[1] - (double)lo[1], dz = (double)hi[2] - (double)lo[2];
    return (dx * dx + dy * dy) + dz * dz;
}

// mu of the linearisation that follows k applied updates: D2, then floor(k / decrease_every) times "if mu > delta2, mu = mu / division_factor".
// Once mu <= delta2 no later step changes it, so the loop leaves there: the trip count is bounded by the schedule, not by k.
MISLAM_FGR_HD inline double fgr_mu(double D2, double delta2, double division_factor, int decrease_every, int k)
{
    double mu = D2;
    const int steps = k / decrease_every;
    for (int s = 0; s < steps && mu > delta2; s++) mu = mu / division_factor;
    return mu;
}

// k of the last linearisation of a loop that ended with `iterations` applied updates: a stop by the stop rule (converged, the cap) follows an
// update, so that linearisation saw one update fewer; every other stop (no pairs, degenerate) and a loop that never ran leave the count as is
inline int fgr_last_k(int iterations, bool stopped_behind_an_update) { return stopped_behind_an_update && iterations > 0 ? iterations - 1 : iterations; }

}  // namespace mislam
