// Host program around cuda-slam_amd/csrc/pose_block.hpp alone (tests/test_pose_block.py builds it plain and under the address and
// undefined-behaviour sanitizers): the state block at a start pose, the check of a caller's transform, the results read out of a block and
// the batch rule of the pose loop, each held to what mi_slam.h promises of them.  Prints "pose_block selftest ok" and returns 0, or names
// the first check that failed.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <limits>

#include "../cuda-slam_amd/csrc/pose_block.hpp"

using namespace mislam;

static int failures = 0;
#define CHECK(cond)                                                                          \
    do {                                                                                     \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); failures++; }   \
    } while (0)

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }
static bool same_bits(float a, float b) { return std::memcmp(&a, &b, sizeof a) == 0; }

// everything of a block but R, t and c0 is zero, bit for bit (the padding word included)
static bool rest_is_zero(const PlaneState& h)
{
    PlaneState z = h;
    std::memset(z.R, 0, sizeof z.R); std::memset(z.t, 0, sizeof z.t); std::memset(z.c0, 0, sizeof z.c0);
    const unsigned char* p = reinterpret_cast<const unsigned char*>(&z);
    for (size_t i = 0; i < sizeof z; i++)
        if (p[i]) return false;
    return h.iterations == 0 && h.done == 0 && h.stop_reason == 0 && h.omega == 0.0 && h.v == 0.0 && h.min_pivot == 0.0;
}

int main()
{
    static_assert(sizeof(PlaneState) == (9 + 3 + 3 + PLANE_ROW + 3) * sizeof(double) + 4 * sizeof(int), "PlaneState: the layout the kernels take by pointer");
    static_assert(PLANE_ROW == 32, "mi_plane_system's out_sums");
    // the named entries of a row: behind the 21 of H, inside the row, g's six ending where E stands, no two the same
    static_assert(PLANE_ROW_G >= 21 && PLANE_ROW_G + 6 == PLANE_ROW_E, "g: six entries between H and E");
    static_assert(PLANE_ROW_E >= 21 && PLANE_ROW_E < PLANE_ROW && PLANE_ROW_AUX >= 21 && PLANE_ROW_AUX < PLANE_ROW && PLANE_ROW_COUNT >= 21 &&
                      PLANE_ROW_COUNT < PLANE_ROW && PLANE_ROW_G < PLANE_ROW,
                  "the named entries lie in [21, 32)");
    static_assert(PLANE_ROW_G != PLANE_ROW_E && PLANE_ROW_G != PLANE_ROW_AUX && PLANE_ROW_G != PLANE_ROW_COUNT && PLANE_ROW_E != PLANE_ROW_AUX &&
                      PLANE_ROW_E != PLANE_ROW_COUNT && PLANE_ROW_AUX != PLANE_ROW_COUNT,
                  "the named entries are distinct");
    static_assert((PLANE_ROW_AUX < PLANE_ROW_G || PLANE_ROW_AUX >= PLANE_ROW_G + 6) && (PLANE_ROW_COUNT < PLANE_ROW_G || PLANE_ROW_COUNT >= PLANE_ROW_G + 6),
                  "neither counter stands inside g");
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    // values no fp32 arithmetic would reproduce by accident: thirds and a denormal
    const float centre[3] = {1.0f / 3.0f, -1234567.875f, 1e-42f};

    {   // a null T: the identity and no translation
        PlaneState h;
        std::memset(&h, 0xa5, sizeof h);
        pose_state_at(nullptr, centre, &h);
        for (int i = 0; i < 9; i++) CHECK(same_bits(h.R[i], i % 4 == 0 ? 1.0 : 0.0));
        for (int i = 0; i < 3; i++) CHECK(same_bits(h.t[i], 0.0));
        for (int i = 0; i < 3; i++) CHECK(same_bits(h.c0[i], (double)centre[i]) && (float)h.c0[i] == centre[i]);
        for (int i = 0; i < PLANE_ROW; i++) CHECK(same_bits(h.sums[i], 0.0));
        CHECK(rest_is_zero(h));
    }
    float T[16];
    for (int i = 0; i < 16; i++) T[i] = (float)(i + 1) + 1.0f / (float)(3 + i);       // 16 distinct values
    {   // 16 distinct values land transposed (T[4 * col + row] -> R[3 * row + col]); t = T[12..14]; the bottom row is not read
        PlaneState h;
        std::memset(&h, 0xa5, sizeof h);
        pose_state_at(T, centre, &h);
        for (int row = 0; row < 3; row++)
            for (int col = 0; col < 3; col++) CHECK(same_bits(h.R[3 * row + col], (double)T[4 * col + row]));
        for (int i = 0; i < 3; i++) CHECK(same_bits(h.t[i], (double)T[12 + i]));
        for (int i = 0; i < 3; i++) CHECK(same_bits(h.c0[i], (double)centre[i]));
        for (int i = 0; i < PLANE_ROW; i++) CHECK(same_bits(h.sums[i], 0.0));
        CHECK(rest_is_zero(h));

        // state -> out_T -> state keeps the bits of fp32-representable values; bottom row 0, 0, 0, 1
        float out[16];
        for (int i = 0; i < 16; i++) out[i] = nan;
        pose_out_T(h, out);
        for (int i = 0; i < 16; i++)
            if (i % 4 != 3) CHECK(same_bits(out[i], T[i]));
        CHECK(same_bits(out[3], 0.f) && same_bits(out[7], 0.f) && same_bits(out[11], 0.f) && same_bits(out[15], 1.f));
        PlaneState back;
        pose_state_at(out, centre, &back);
        CHECK(std::memcmp(back.R, h.R, sizeof h.R) == 0 && std::memcmp(back.t, h.t, sizeof h.t) == 0);
    }
    {   // the transform check: each of the 12 read entries, NaN and both infinities, by its index; the bottom row is free
        CHECK(pose_bad_entry(T) == -1);
        for (int i = 0; i < 16; i++)
            for (float bad : {nan, inf, -inf}) {
                float U[16];
                std::memcpy(U, T, sizeof U);
                U[i] = bad;
                CHECK(pose_bad_entry(U) == (i % 4 == 3 ? -1 : i));
            }
        float U[16];
        std::memcpy(U, T, sizeof U);
        U[3] = U[7] = U[11] = U[15] = nan;
        CHECK(pose_bad_entry(U) == -1);
        U[14] = nan; U[5] = inf;                 // the lowest index is the one named
        CHECK(pose_bad_entry(U) == 5);
    }
    {   // the error: sums[27] / sums[29] rounded to fp32 once, and exactly 0 without a pair
        PlaneState h;
        pose_state_at(nullptr, centre, &h);
        h.sums[27] = 1.0; h.sums[29] = 3.0;
        CHECK(same_bits(pose_error(h), (float)(1.0 / 3.0)));
        h.sums[27] = 0.1; h.sums[29] = 7.0;
        CHECK(same_bits(pose_error(h), (float)(0.1 / 7.0)));
        h.sums[27] = 5.0; h.sums[29] = 0.0;
        CHECK(same_bits(pose_error(h), 0.f));
        h.sums[27] = (double)nan; h.sums[29] = 0.0;
        CHECK(same_bits(pose_error(h), 0.f));
    }
    {   // the error reads E and COUNT by their names and nothing else: every other entry of the block is poisoned (NaN, or bytes of 0xa5)
        PlaneState h;
        std::memset(&h, 0xa5, sizeof h);
        for (int i = 0; i < PLANE_ROW; i++) h.sums[i] = (double)nan;
        h.sums[PLANE_ROW_E] = 0.1; h.sums[PLANE_ROW_COUNT] = 7.0;
        CHECK(same_bits(pose_error(h), (float)(0.1 / 7.0)));
        h.sums[PLANE_ROW_E] = 5.0; h.sums[PLANE_ROW_COUNT] = 0.0;
        CHECK(same_bits(pose_error(h), 0.f));
        // ... and a poisoned E or COUNT shows: the two are read
        h.sums[PLANE_ROW_E] = (double)nan; h.sums[PLANE_ROW_COUNT] = 7.0;
        CHECK(std::isnan(pose_error(h)));
        h.sums[PLANE_ROW_E] = 0.1; h.sums[PLANE_ROW_COUNT] = (double)nan;
        CHECK(same_bits(pose_error(h), 0.f));          // (NaN > 0 is false: no pair)
    }
    {   // the batch rule
        CHECK(pose_batch(0) == 4);
        for (int s : {1, 2, 3, 4, 5, 50, 1000000}) CHECK(pose_batch(s) == s);
        CHECK(pose_batch_todo(4, 7, 0) == 4 && pose_batch_todo(4, 7, 4) == 3);      // 7 iterations in batches of 4: 4, then 3
        CHECK(pose_batch_todo(4, 8, 4) == 4 && pose_batch_todo(1, 7, 6) == 1 && pose_batch_todo(50, 7, 0) == 7);
        int enqueued = 0, batches = 0;
        while (enqueued < 7) { enqueued += pose_batch_todo(pose_batch(0), 7, enqueued); batches++; }
        CHECK(enqueued == 7 && batches == 2);
    }
    if (failures) { std::printf("pose_block selftest: %d checks failed\n", failures); return 1; }
    std::printf("pose_block selftest ok\n");
    return 0;
}
