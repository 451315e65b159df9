// Host program around cuda-slam_amd/csrc/mls_fit.hpp alone (tests/test_mls_fit.py builds it plain and under the address and
// undefined-behaviour sanitizers).  It reads records from stdin and prints one line per record with %.17g:
//   f  n[3]                                  -> u[3] v[3]                                                        mls_frame
//   c  n[3] o[3] s2 count d[count][3]        -> ok (1 / 0), the smallest pivot, the six coefficients             mls_frame, mls_basis, plane_solve6
//   q  order s2 q[3] count d[count][3]       -> status, the smallest pivot, xyz[3], normal[3], n[3], o[3], curvature, lambda[3]
//                                                                                                                 the sums, mls_plane, mls_basis, mls_project
// d = p_j - q, as the kernel's sinks form it.
#include <cstdio>
#include <vector>

#include "../cuda-slam_amd/csrc/mls_fit.hpp"

using namespace mislam;

static bool read(double* out, int count)
{
    for (int i = 0; i < count; i++)
        if (std::scanf("%lf", &out[i]) != 1) return false;
    return true;
}

static bool read_points(std::vector<double>& d)
{
    int count;
    if (std::scanf("%d", &count) != 1 || count < 0 || count > 100000) return false;
    d.resize(3 * (size_t)count);
    return read(d.data(), 3 * count);
}

int main()
{
    char kind;
    long long records = 0;
    std::vector<double> d;
    while (std::scanf(" %c", &kind) == 1) {
        if (kind == 'f') {
            double n[3], u[3], v[3];
            if (!read(n, 3)) { std::fprintf(stderr, "mls_fit_selftest: short frame record\n"); return 2; }
            mls_frame(n, u, v);
            std::printf("%.17g %.17g %.17g %.17g %.17g %.17g\n", u[0], u[1], u[2], v[0], v[1], v[2]);
        } else if (kind == 'c') {
            MlsPlane p{};
            double s2;
            if (!read(p.n, 3) || !read(p.o, 3) || !read(&s2, 1) || !read_points(d)) { std::fprintf(stderr, "mls_fit_selftest: short basis record\n"); return 2; }
            mls_frame(p.n, p.u, p.v);
            double A[21] = {0}, g[6] = {0}, x[6] = {0, 0, 0, 0, 0, 0}, min_pivot = -1.0;
            for (size_t j = 0; j < d.size() / 3; j++) mls_basis(p, d[3 * j], d[3 * j + 1], d[3 * j + 2], s2, A, g);
            const bool ok = plane_solve6(A, g, x, &min_pivot);
            std::printf("%d %.17g", ok ? 1 : 0, min_pivot);
            for (int i = 0; i < 6; i++) std::printf(" %.17g", ok ? -x[i] : 0.0);
            std::printf("\n");
        } else if (kind == 'q') {
            int order;
            double s2, q[3];
            if (std::scanf("%d", &order) != 1 || !read(&s2, 1) || !read(q, 3) || !read_points(d) || d.empty()) {
                std::fprintf(stderr, "mls_fit_selftest: short query record\n");
                return 2;
            }
            const int c = (int)(d.size() / 3);
            double S[3] = {0, 0, 0}, Q[6] = {0, 0, 0, 0, 0, 0};
            for (int j = 0; j < c; j++) {
                const double dx = d[3 * j], dy = d[3 * j + 1], dz = d[3 * j + 2];
                S[0] += dx; S[1] += dy; S[2] += dz;
                Q[0] += dx * dx; Q[1] += dx * dy; Q[2] += dx * dz;
                Q[3] += dy * dy; Q[4] += dy * dz; Q[5] += dz * dz;
            }
            MlsPlane p;
            mls_plane(S, Q, c, p);
            double A[21] = {0}, g[6] = {0}, xyz[3], normal[3], min_pivot = -1.0;
            if (order == 2 && c >= MLS_QUADRATIC_MIN)
                for (int j = 0; j < c; j++) mls_basis(p, d[3 * j], d[3 * j + 1], d[3 * j + 2], s2, A, g);
            const int status = mls_project(p, q, order, c, A, g, xyz, normal, &min_pivot);
            std::printf("%d %.17g", status, min_pivot);
            for (int k = 0; k < 3; k++) std::printf(" %.17g", xyz[k]);
            for (int k = 0; k < 3; k++) std::printf(" %.17g", normal[k]);
            for (int k = 0; k < 3; k++) std::printf(" %.17g", p.n[k]);
            for (int k = 0; k < 3; k++) std::printf(" %.17g", p.o[k]);
            std::printf(" %.17g %.17g %.17g %.17g\n", p.curvature, p.lambda[0], p.lambda[1], p.lambda[2]);
        } else {
            std::fprintf(stderr, "mls_fit_selftest: unknown record '%c'\n", kind);
            return 2;
        }
        records++;
    }
    std::fprintf(stderr, "mls_fit_selftest: %lld records\n", records);
    return 0;
}
