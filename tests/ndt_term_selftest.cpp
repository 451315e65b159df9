// Host program around cuda-slam_amd/csrc/ndt_term.hpp, the header alone (no HIP runtime): tests/test_ndt_term.py builds it plain and
// under the address and undefined-behaviour sanitizers.  Input: a file of rows "q(3) mu(3) M(6) h k", every number as %.17g.  Output, one
// row per input row: "ok d(3) Md(3) m e w" from ndt_term, then the same twelve numbers from the plain-C restatement below, all as %.17g
// (ok: 0 or 1; the numbers behind a 0 are printed as 0).  It also folds every term of the file into one NdtPointSums and prints that
// as the last row, "A(6) b(3) E terms", beside the restatement's.
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <vector>

#include "../cuda-slam_amd/csrc/ndt_term.hpp"

namespace {

// the rule of include/mi_slam.h, written out with scalars
bool plain_term(const double* q, const double* mu, const double* M, double h, double k, double out[12])
{
    if (M[0] == 0 && M[1] == 0 && M[2] == 0 && M[3] == 0 && M[4] == 0 && M[5] == 0) return false;
    const double dx = q[0] - mu[0], dy = q[1] - mu[1], dz = q[2] - mu[2];
    double t = M[0] * dx; t = t + M[1] * dy; const double a0 = t + M[2] * dz;
    t = M[1] * dx; t = t + M[3] * dy; const double a1 = t + M[4] * dz;
    t = M[2] * dx; t = t + M[4] * dy; const double a2 = t + M[5] * dz;
    t = dx * a0; t = t + dy * a1; const double m = t + dz * a2;
    if (std::isnan(m) || std::isinf(m) || m < 0) return false;
    const double e = std::exp(h * m);
    const double v[12] = {1, dx, dy, dz, a0, a1, a2, m, e, k * e, 0, 0};
    for (int i = 0; i < 12; i++) out[i] = v[i];
    return true;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc != 2) { std::fprintf(stderr, "usage: %s rows.txt\n", argv[0]); return 2; }
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    std::vector<double> row(14);
    mislam::NdtPointSums sums;
    mislam::ndt_point_clear(&sums);
    double pA[6] = {0, 0, 0, 0, 0, 0}, pb[3] = {0, 0, 0}, pE = 0;
    int pterms = 0;
    for (;;) {
        int got = 0;
        for (int i = 0; i < 14; i++) got += std::fscanf(f, "%lf", &row[i]) == 1 ? 1 : 0;
        if (got == 0) break;
        if (got != 14) { std::fprintf(stderr, "short row\n"); std::fclose(f); return 2; }
        const double *q = &row[0], *mu = &row[3], *M = &row[6], h = row[12], k = row[13];
        mislam::NdtTerm t;
        double a[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, b[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        if (mislam::ndt_term(q, mu, M, h, k, &t)) {
            const double v[10] = {1, t.d[0], t.d[1], t.d[2], t.Md[0], t.Md[1], t.Md[2], t.m, t.e, t.w};
            for (int i = 0; i < 10; i++) a[i] = v[i];
            mislam::ndt_point_add(&sums, M, t);
        }
        if (plain_term(q, mu, M, h, k, b)) {
            for (int i = 0; i < 6; i++) { const double p = b[9] * M[i]; pA[i] = pA[i] + p; }
            for (int i = 0; i < 3; i++) { const double p = b[9] * b[4 + i]; pb[i] = pb[i] + p; }
            pE = pE + b[8];
            pterms++;
        }
        for (int i = 0; i < 10; i++) std::printf("%.17g ", a[i]);
        for (int i = 0; i < 10; i++) std::printf("%.17g%c", b[i], i == 9 ? '\n' : ' ');
    }
    std::fclose(f);
    for (int i = 0; i < 6; i++) std::printf("%.17g ", sums.A[i]);
    for (int i = 0; i < 3; i++) std::printf("%.17g ", sums.b[i]);
    std::printf("%.17g %d ", sums.E, sums.terms);
    for (int i = 0; i < 6; i++) std::printf("%.17g ", pA[i]);
    for (int i = 0; i < 3; i++) std::printf("%.17g ", pb[i]);
    std::printf("%.17g %d\n", pE, pterms);
    return 0;
}
