// Host program around cuda-slam_amd/csrc/eig3.hpp alone (tests/test_eig3.py builds it plain and under the address and undefined-behaviour
// sanitizers): reads symmetric 3x3 matrices from stdin, six numbers each (a00 a01 a02 a11 a12 a22), and prints per matrix one line of
// twelve numbers, the three eigenvalues and then V row by row, with %.17g.
#include <cstdio>

#include "../cuda-slam_amd/csrc/eig3.hpp"

int main()
{
    double a[6];
    long long count = 0;
    for (;;) {
        int got = 0;
        while (got < 6 && std::scanf("%lf", &a[got]) == 1) got++;
        if (got == 0) break;
        if (got != 6) { std::fprintf(stderr, "eig3_selftest: %d numbers left over, a matrix takes 6\n", got); return 2; }
        double lambda[3], v[9];
        mislam::eig3_symmetric<double>(a, lambda, v);
        std::printf("%.17g %.17g %.17g", lambda[0], lambda[1], lambda[2]);
        for (int i = 0; i < 9; i++) std::printf(" %.17g", v[i]);
        std::printf("\n");
        count++;
    }
    std::fprintf(stderr, "eig3_selftest: %lld matrices\n", count);
    return 0;
}
