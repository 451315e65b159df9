// Host program around cuda-slam_amd/csrc/eval_block.hpp alone (tests/test_eval_block.py builds it plain and under the address and
// undefined-behaviour sanitizers): the fitness, the inlier RMSE and the 21 -> 36 expansion of mi_evaluate_registration, each held to what
// mi_slam.h promises of them.  Prints "eval_block selftest ok" and returns 0, or names the first check that failed.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>

#include "../cuda-slam_amd/csrc/eval_block.hpp"

using namespace mislam;

static int failures = 0;
#define CHECK(cond)                                                                          \
    do {                                                                                     \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); failures++; }   \
    } while (0)

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

int main()
{
    const double nan = std::numeric_limits<double>::quiet_NaN();
    {   // the slots: the upper triangle row by row, as pose_row_write counts them, and symmetric
        int k = 0;
        for (int i = 0; i < 6; i++)
            for (int j = i; j < 6; j++) {
                CHECK(eval_triangle_slot(i, j) == k && eval_triangle_slot(j, i) == k);
                k++;
            }
        CHECK(k == PLANE_ROW_G);
    }
    double sums[PLANE_ROW];
    for (int i = 0; i < PLANE_ROW; i++) sums[i] = nan;                       // whatever is not read is poison
    for (int i = 0; i < 21; i++) sums[i] = 1.0 / (double)(3 + i) - 0.1;      // 21 distinct values, some negative
    sums[PLANE_ROW_E] = 0.7; sums[PLANE_ROW_COUNT] = 3.0;
    {   // the expansion: the same bits at (i, j) and (j, i), the diagonal where the triangle has it
        double out[36];
        for (double& v : out) v = nan;
        eval_information(sums, out);
        int k = 0;
        for (int i = 0; i < 6; i++)
            for (int j = i; j < 6; j++) {
                CHECK(same_bits(out[6 * i + j], sums[k]) && same_bits(out[6 * j + i], sums[k]));
                k++;
            }
        // a signed zero keeps its sign
        double z[PLANE_ROW] = {0};
        z[1] = -0.0; z[PLANE_ROW_COUNT] = 1.0;
        eval_information(z, out);
        CHECK(same_bits(out[1], -0.0) && same_bits(out[6], -0.0) && same_bits(out[0], 0.0));
    }
    {   // fitness and RMSE: one division; one division and one root; they read COUNT and E by name and nothing else
        CHECK(same_bits(eval_fitness(sums, 7), 3.0 / 7.0));
        CHECK(same_bits(eval_fitness(sums, 3), 1.0));
        CHECK(same_bits(eval_inlier_rmse(sums), std::sqrt(0.7 / 3.0)));
        sums[PLANE_ROW_E] = 0.0;
        CHECK(same_bits(eval_inlier_rmse(sums), 0.0));
    }
    {   // no pair: fitness 0, RMSE 0 whatever E holds, the matrix all +0 whatever the triangle holds
        sums[PLANE_ROW_COUNT] = 0.0; sums[PLANE_ROW_E] = nan;
        double out[36];
        for (double& v : out) v = nan;
        eval_information(sums, out);
        for (double v : out) CHECK(same_bits(v, 0.0));
        CHECK(same_bits(eval_fitness(sums, 5), 0.0) && same_bits(eval_inlier_rmse(sums), 0.0));
    }
    if (failures) { std::printf("eval_block selftest: %d checks failed\n", failures); return 1; }
    std::printf("eval_block selftest ok\n");
    return 0;
}
