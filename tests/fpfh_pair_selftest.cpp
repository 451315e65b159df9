// Host program around cuda-slam_amd/csrc/fpfh_pair.hpp alone (tests/test_fpfh_pair.py builds it plain and under the address and
// undefined-behaviour sanitizers, with -ffp-contract=off like the library): reads pairs from the file named on the command line, twelve
// numbers each (p_i, n_i, p_j, n_j), and prints per pair one line: theta, alpha, phi with %.17g and then their three bins.
#include <cstdio>

#include "../cuda-slam_amd/csrc/fpfh_pair.hpp"

int main(int argc, char** argv)
{
    if (argc != 2) { std::fprintf(stderr, "usage: fpfh_pair_selftest <file of pairs>\n"); return 2; }
    std::FILE* in = std::fopen(argv[1], "r");
    if (!in) { std::fprintf(stderr, "fpfh_pair_selftest: cannot open %s\n", argv[1]); return 2; }
    double a[12];
    long long count = 0;
    for (;;) {
        int got = 0;
        while (got < 12 && std::fscanf(in, "%lf", &a[got]) == 1) got++;
        if (got == 0) break;
        if (got != 12) { std::fprintf(stderr, "fpfh_pair_selftest: %d numbers left over, a pair takes 12\n", got); std::fclose(in); return 2; }
        double theta, alpha, phi;
        mislam::fpfh_pair_features(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9], a[10], a[11], theta, alpha, phi);
        std::printf("%.17g %.17g %.17g %d %d %d\n", theta, alpha, phi, mislam::fpfh_bin_angle(theta), mislam::fpfh_bin_cosine(alpha) + mislam::FPFH_BINS,
                    mislam::fpfh_bin_cosine(phi) + 2 * mislam::FPFH_BINS);
        count++;
    }
    std::fclose(in);
    std::fprintf(stderr, "fpfh_pair_selftest: %lld pairs\n", count);
    return 0;
}
