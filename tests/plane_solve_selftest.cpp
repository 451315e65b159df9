// Host program around cuda-slam_amd/csrc/plane_solve.hpp alone (tests/test_plane_solve.py builds it plain and under the address and
// undefined-behaviour sanitizers).  It reads records from stdin and prints one line per record with %.17g:
//   s  a[21] g[6]                      -> ok (1 / 0), the smallest pivot, x[6] (zeros where not ok)      plane_solve6
//   p  w[3] v[3] c0[3] R[9] t[3]       -> dR[9], the composed R[9], the composed t[3]                    plane_rodrigues, plane_compose
#include <cstdio>

#include "../cuda-slam_amd/csrc/plane_solve.hpp"

static bool read(double* out, int count)
{
    for (int i = 0; i < count; i++)
        if (std::scanf("%lf", &out[i]) != 1) return false;
    return true;
}

int main()
{
    char kind;
    long long records = 0;
    while (std::scanf(" %c", &kind) == 1) {
        if (kind == 's') {
            double a[21], g[6], x[6] = {0, 0, 0, 0, 0, 0}, min_pivot = -1.0;
            if (!read(a, 21) || !read(g, 6)) { std::fprintf(stderr, "plane_solve_selftest: short solve record\n"); return 2; }
            const bool ok = mislam::plane_solve6(a, g, x, &min_pivot);
            std::printf("%d %.17g", ok ? 1 : 0, min_pivot);
            for (int i = 0; i < 6; i++) std::printf(" %.17g", ok ? x[i] : 0.0);
            std::printf("\n");
        } else if (kind == 'p') {
            double w[3], v[3], c0[3], R[9], t[3], dR[9];
            if (!read(w, 3) || !read(v, 3) || !read(c0, 3) || !read(R, 9) || !read(t, 3)) { std::fprintf(stderr, "plane_solve_selftest: short pose record\n"); return 2; }
            mislam::plane_rodrigues(w, dR);
            mislam::plane_compose(dR, v, c0, R, t);
            for (int i = 0; i < 9; i++) std::printf("%.17g ", dR[i]);
            for (int i = 0; i < 9; i++) std::printf("%.17g ", R[i]);
            std::printf("%.17g %.17g %.17g\n", t[0], t[1], t[2]);
        } else {
            std::fprintf(stderr, "plane_solve_selftest: unknown record '%c'\n", kind);
            return 2;
        }
        records++;
    }
    std::fprintf(stderr, "plane_solve_selftest: %lld records\n", records);
    return 0;
}
