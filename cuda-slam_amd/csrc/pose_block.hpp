// The state block of the pose loop that plane ICP, generalized ICP and NDT share (K16, K17, K31; the loop: pose_loop.hip) and the host
// arithmetic on it that needs no device: the check of a caller's transform, the block at a start pose, the results read out of it, the batch
// rule.  Nothing of HIP is included, so that tests/pose_block_selftest.cpp can hold it to its contract on the host alone.
#pragma once
#include <cmath>
#include <cstring>

namespace mislam {

// A row: what a step kernel sums over the 64 moving points of one wave (pose_row_write, pose_step.hpp), and a system: the rows' sum.
//   [0, 21)                        H, the upper triangle of the 6 x 6 matrix row by row: sum J J^T (K16), sum J^T M J (K17, K31)
//   [PLANE_ROW_G, PLANE_ROW_G + 6) g: sum J r (K16), sum J^T M d (K17), sum J^T b (K31)
//   [PLANE_ROW_E]                  the objective: sum r^2 (K16), sum d^T M d (K17), sum e (K31)
//   [PLANE_ROW_AUX]                sum d2 over the pairs (K16, K17); points with a term (K31)
//   [PLANE_ROW_COUNT]              pairs (K16, K17); terms (K31)
//   [30, 32)                       0
constexpr int PLANE_ROW = 32;                // doubles per row and per system: mi_plane_system's out_sums
constexpr int PLANE_ROW_G = 21;              // (= the entries of H before it)
constexpr int PLANE_ROW_E = 27;
constexpr int PLANE_ROW_AUX = 28;
constexpr int PLANE_ROW_COUNT = 29;

// Device-resident loop state of one plane registration.  The host only ever copies it back; every decision is taken on the device.
struct PlaneState {
    double R[9];             // running rotation, ROW-major
    double t[3];             // running translation
    double c0[3];            // the centre the moments are taken about, promoted from its fp32 value
    double sums[PLANE_ROW];  // the last linearisation's system
    double omega, v;         // lengths of the last update's two halves
    double min_pivot;        // smallest pivot of the last solve (0: a bad diagonal)
    int iterations;          // updates applied
    int done;
    int stop_reason;
    int pad;
};

// the first entry of a column-major 4 x 4 transform that is read and not finite, or -1: the rotation block and the translation column are
// read, the bottom row (3, 7, 11, 15) never is
inline int pose_bad_entry(const float T[16])
{
    for (int i = 0; i < 16; i++)
        if (i % 4 != 3 && !std::isfinite(T[i])) return i;
    return -1;
}

// the block a loop starts from: the pose T (null: the identity), the centre, everything else zero
inline void pose_state_at(const float* T, const float centre[3], PlaneState* h)
{
    std::memset(h, 0, sizeof *h);
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) h->R[3 * i + j] = T ? (double)T[4 * j + i] : (i == j ? 1.0 : 0.0);      // column-major in, row-major kept
        h->t[i] = T ? (double)T[12 + i] : 0.0;
        h->c0[i] = (double)centre[i];
    }
}

// the pose of a block as a caller's transform: column-major, bottom row 0, 0, 0, 1
inline void pose_out_T(const PlaneState& h, float out_T[16])
{
    for (int i = 0; i < 16; i++) out_T[i] = 0.f;
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) out_T[4 * j + i] = (float)h.R[3 * i + j];
        out_T[12 + i] = (float)h.t[i];
    }
    out_T[15] = 1.f;
}

// the last linearisation's objective per pair (or term); 0 where there was none
inline float pose_error(const PlaneState& h) { return h.sums[PLANE_ROW_COUNT] > 0.0 ? (float)(h.sums[PLANE_ROW_E] / h.sums[PLANE_ROW_COUNT]) : 0.f; }

// iterations enqueued between two host reads of the state, and how many of them the next batch holds under the cap
inline int pose_batch(int sync_every) { return sync_every > 0 ? sync_every : 4; }
inline int pose_batch_todo(int batch, int max_iterations, int enqueued) { return batch < max_iterations - enqueued ? batch : max_iterations - enqueued; }

}  // namespace mislam
