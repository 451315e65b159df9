// The pose loop of plane ICP, generalized ICP and NDT, stated once for mi_icp_plane_register, mi_icp_gicp_register, mi_ndt_register and their
// *_system probes (declared in context.h; the loop itself and an iteration's two launches are templates there, over the driver's step launch).
// The three step kernels write the same rows and read the same device state block, and plane_reduce_solve stands behind all of them, so
// everything behind "the step kernel's arguments are complete" is stated here: the checks of a caller's transform and loop fields, the reserves
// and the shape check of the rows, slabs, state and out_idx, the state block at the start pose (pose_block.hpp) and its upload, the read-back,
// and the results of both kinds of call.  A driver keeps what concerns its own arrays and its step.  `who`: the entry point's name, for messages.
#include <hip/hip_runtime.h>

#include "context.h"

namespace mislam {

static_assert(MI_STOP_DEGENERATE == MI_STOP_DEGENERATE_, "kernels.h mirrors MI_STOP_DEGENERATE");
static_assert(MI_STOP_NO_PAIRS == MI_STOP_NO_PAIRS_ && MI_STOP_CONVERGED == MI_STOP_CONVERGED_ && MI_STOP_MAX_ITERATIONS == MI_STOP_MAX_ITERATIONS_, "kernels.h mirrors MI_STOP_*");

int pose_check_transform(const char* who, const float* T)
{
    const int bad = T ? pose_bad_entry(T) : -1;
    if (bad >= 0) { set_error("%s: transform entry %d is not finite (%g)", who, bad, (double)T[bad]); return MI_ERR_INVALID_ARG; }
    return MI_OK;
}

int pose_check_fields(const char* who, const PoseLoopFields& p)
{
    if (!(p.eps_rotation >= 0.f) || !(p.eps_translation >= 0.f)) {
        set_error("%s: eps_rotation %g or eps_translation %g is NaN or negative", who, (double)p.eps_rotation, (double)p.eps_translation);
        return MI_ERR_INVALID_ARG;
    }
    if (p.max_iterations < 0) { set_error("%s: max_iterations %d is negative (there is no unbounded mode)", who, p.max_iterations); return MI_ERR_INVALID_ARG; }
    if (p.sync_every < 0) { set_error("%s: sync_every %d is negative", who, p.sync_every); return MI_ERR_INVALID_ARG; }
    return MI_OK;
}

int pose_loop_reserve(PoseLoopBuffers& b, int n, bool want_idx)
{
    const int nrows = plane_row_count(n), nparts = plane_part_count(nrows);
    MI_TRY(b.rows.reserve((size_t)nrows * PLANE_ROW));
    if (nparts > 0) MI_TRY(b.parts.reserve((size_t)nparts * PLANE_ROW));
    MI_TRY(b.state.reserve(1));
    if (want_idx) MI_TRY(b.out_idx.reserve((size_t)n));
    return MI_OK;
}

bool pose_loop_fits(const PoseLoopBuffers& b, int n, bool want_idx)
{
    const int nrows = plane_row_count(n), nparts = plane_part_count(nrows);
    return b.rows.cap >= (size_t)nrows * PLANE_ROW && b.state.cap >= 1 && (nparts == 0 || b.parts.cap >= (size_t)nparts * PLANE_ROW) &&
           (!want_idx || b.out_idx.cap >= (size_t)n);
}

int pose_loop_upload_state(mi_ctx* c, PoseLoopBuffers& b, StageClock& clock, const float* T, const float centre[3], PlaneState* h)
{
    pose_state_at(T, centre, h);
    MI_TRY(host_to_device(c, b.state.p, h, sizeof *h));
    return clock.mark(1);
}

int pose_loop_read_state(mi_ctx* c, PoseLoopBuffers& b, PlaneState* h)
{
    MI_HIP(hipMemcpyAsync(h, b.state.p, sizeof *h, hipMemcpyDeviceToHost, c->stream));
    MI_HIP(hipStreamSynchronize(c->stream));
    return MI_OK;
}

int pose_loop_results(StageClock& clock, const PlaneState& h, float out_T[16], int* iterations, float* error, int* stop_reason)
{
    pose_out_T(h, out_T);
    if (iterations) *iterations = h.iterations;
    if (error) *error = pose_error(h);
    if (stop_reason) *stop_reason = h.stop_reason;
    MI_TRY(clock.mark(6));
    clock.finish();
    return MI_OK;
}

int pose_loop_system_finish(mi_ctx* c, StageClock& clock, const PlaneState& h, double out_sums[PLANE_ROW], float out_centre[3])
{
    MI_HIP(hipStreamSynchronize(c->stream));
    for (int i = 0; i < PLANE_ROW; i++) out_sums[i] = h.sums[i];
    if (out_centre)
        for (int i = 0; i < 3; i++) out_centre[i] = (float)h.c0[i];
    MI_TRY(clock.mark(6));
    clock.finish();
    return MI_OK;
}

}  // namespace mislam
