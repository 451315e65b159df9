// Host program around cuda-slam_amd/csrc/color_terms.hpp alone (tests/test_color_terms.py builds it plain and under the address and
// undefined-behaviour sanitizers, with -ffp-contract=off like the library).  color_terms_selftest <mode> <file>, every number printed with %.17g:
//   pairs  18 numbers a line -- q, a, c0, n, g (three each), Ia, Ib, lambda -- -> the pair's 28 entries: 21 of H, 6 of g, e
//   solve  9 numbers a line -- M (xx, xy, xz, yy, yz, zz), b -- -> d and 1 where the solve stood, 0 where it gave zeros
//   sums   23 numbers a line -- n, then five neighbours of e (three) and delta -- -> M and b behind the constraint with count 5
#include <cstdio>
#include <cstring>

#include "../cuda-slam_amd/csrc/color_terms.hpp"

int main(int argc, char** argv)
{
    if (argc != 3) { std::fprintf(stderr, "usage: color_terms_selftest pairs|solve|sums <file>\n"); return 2; }
    const int per = !std::strcmp(argv[1], "pairs") ? 18 : (!std::strcmp(argv[1], "solve") ? 9 : (!std::strcmp(argv[1], "sums") ? 23 : 0));
    if (per == 0) { std::fprintf(stderr, "color_terms_selftest: unknown mode %s\n", argv[1]); return 2; }
    std::FILE* in = std::fopen(argv[2], "r");
    if (!in) { std::fprintf(stderr, "color_terms_selftest: cannot open %s\n", argv[2]); return 2; }
    double v[23];
    long long count = 0;
    for (;;) {
        int got = 0;
        while (got < per && std::fscanf(in, "%lf", &v[got]) == 1) got++;
        if (got == 0) break;
        if (got != per) { std::fprintf(stderr, "color_terms_selftest: %d numbers left over, a line takes %d\n", got, per); std::fclose(in); return 2; }
        if (per == 18) {
            const double q[3] = {v[0], v[1], v[2]}, a[3] = {v[3], v[4], v[5]}, c0[3] = {v[6], v[7], v[8]}, n[3] = {v[9], v[10], v[11]}, g[3] = {v[12], v[13], v[14]};
            mislam::ColorPair p;
            mislam::color_pair_none(p);
            mislam::color_pair_terms(q, a, c0, n, g, v[15], v[16], p);
            const double lg = (double)(float)v[17], lc = 1.0 - lg;
            for (int i = 0; i < 6; i++)
                for (int j = i; j < 6; j++) std::printf("%.17g ", mislam::color_pair_h(p, lg, lc, i, j));
            for (int i = 0; i < 6; i++) std::printf("%.17g ", mislam::color_pair_g(p, lg, lc, i));
            std::printf("%.17g\n", mislam::color_pair_e(p, lg, lc));
        } else if (per == 9) {
            const double M[6] = {v[0], v[1], v[2], v[3], v[4], v[5]}, b[3] = {v[6], v[7], v[8]};
            double d[3];
            const bool ok = mislam::color_gradient_solve(M, b, d);
            std::printf("%.17g %.17g %.17g %d\n", d[0], d[1], d[2], ok ? 1 : 0);
        } else {
            const double n[3] = {v[0], v[1], v[2]};
            double M[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, b[3] = {0.0, 0.0, 0.0};
            for (int k = 0; k < 5; k++) mislam::color_gradient_add(n, v[3 + 4 * k], v[4 + 4 * k], v[5 + 4 * k], v[6 + 4 * k], M, b);
            mislam::color_gradient_constrain(n, 5, M);
            std::printf("%.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", M[0], M[1], M[2], M[3], M[4], M[5], b[0], b[1], b[2]);
        }
        count++;
    }
    std::fclose(in);
    std::fprintf(stderr, "color_terms_selftest: %lld lines\n", count);
    return 0;
}
