// K56-K63 building block: the arithmetic of one pose-graph edge (mi_pose_graph_optimize), usable from one GPU lane and from host code (the
// edge kernel of pose_graph_kernels.hip; tests/pose_graph_terms_selftest.cpp compiles this header alone with a host compiler).  The single
// statement of the rules mi_slam.h gives under "Error", "Residual", "Jacobians", "Terms" and "Line process"; everything is fp64, every
// matrix row-major, a pose 12 numbers: R (9), then t (3).
//
//   pg_inverse     (R, t)^-1 = (R^T, -(R^T t))
//   pg_product     (Ra, ta) (Rb, tb) = (Ra Rb, Ra tb + ta), every entry ((a0 b0 + a1 b1) + a2 b2) [+ t]
//   pg_log_so3     s = half the antisymmetric part of R, omega = s * (theta / |s|), theta = atan2(|s|, (trace - 1) / 2); below |s| = 1e-8, s itself
//   pg_adjoint     A = Ad(T_t^-1) = [[Q, 0], [[t']x Q, Q]], Q = R_t^T, t' = -(Q t_t)
//   pg_edge_terms  E = T_t^-1 T_s Z^-1 (Z is inverted here, from the measurement as given), r = (log_SO3(R_E), t_E), u = Lambda r,
//                  chi2 = r . u, the line process' weight w and share of the cost, M = w A^T Lambda A (upper triangle, 21 numbers) and
//                  h = w A^T u.  Lambda comes as the 21 numbers of its upper triangle.
//   pg_list_slot   the order of a node's incidence list: ascending edge index, the source side of an edge before its target side
// Every loop has constant bounds and is unrolled on the device, so every index is static there.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MISLAM_PG_HD __host__ __device__
#define MISLAM_PG_UNROLL _Pragma("unroll")
#else
#define MISLAM_PG_HD
#define MISLAM_PG_UNROLL
#endif

#include <cmath>

namespace mislam {

constexpr double PG_LOG_SMALL = 1e-8;         // |s| under which log_SO3 returns the antisymmetric part itself
constexpr int PG_POSE = 12;                   // R row-major, then t
constexpr int PG_TRI = 21;                    // the upper triangle of a symmetric 6 x 6, row-major
constexpr int PG_LONG_LIST = 64;              // an incidence list longer than this is summed by one wave (pose_graph_kernels.hip)

MISLAM_PG_HD inline void pg_inverse(const double (&R)[9], const double (&t)[3], double (&Ri)[9], double (&ti)[3])
{
    MISLAM_PG_UNROLL
    for (int i = 0; i < 3; i++) {
        MISLAM_PG_UNROLL
        for (int j = 0; j < 3; j++) Ri[3 * i + j] = R[3 * j + i];
    }
    MISLAM_PG_UNROLL
    for (int i = 0; i < 3; i++) ti[i] = -((Ri[3 * i] * t[0] + Ri[3 * i + 1] * t[1]) + Ri[3 * i + 2] * t[2]);
}

MISLAM_PG_HD inline void pg_product(const double (&Ra)[9], const double (&ta)[3], const double (&Rb)[9], const double (&tb)[3], double (&R)[9], double (&t)[3])
{
    MISLAM_PG_UNROLL
    for (int i = 0; i < 3; i++) {
        MISLAM_PG_UNROLL
        for (int j = 0; j < 3; j++) R[3 * i + j] = (Ra[3 * i] * Rb[j] + Ra[3 * i + 1] * Rb[3 + j]) + Ra[3 * i + 2] * Rb[6 + j];
        t[i] = ((Ra[3 * i] * tb[0] + Ra[3 * i + 1] * tb[1]) + Ra[3 * i + 2] * tb[2]) + ta[i];
    }
}

MISLAM_PG_HD inline void pg_log_so3(const double (&R)[9], double (&w)[3])
{
    using std::atan2;
    using std::sqrt;
    const double s[3] = {0.5 * (R[7] - R[5]), 0.5 * (R[2] - R[6]), 0.5 * (R[3] - R[1])};
    const double n = sqrt((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]);
    const double c = 0.5 * (((R[0] + R[4]) + R[8]) - 1.0);
    double k = 1.0;
    if (!(n < PG_LOG_SMALL)) k = atan2(n, c) / n;
    MISLAM_PG_UNROLL
    for (int i = 0; i < 3; i++) w[i] = s[i] * k;
}

// A = Ad((R, t)^-1) of a target pose (R, t), all 36 entries (the upper right block is 0)
MISLAM_PG_HD inline void pg_adjoint(const double (&R)[9], const double (&t)[3], double (&A)[36])
{
    double Q[9], tp[3];
    pg_inverse(R, t, Q, tp);
    // P = [t']x Q
    double P[9];
    MISLAM_PG_UNROLL
    for (int j = 0; j < 3; j++) {
        P[j] = tp[1] * Q[6 + j] - tp[2] * Q[3 + j];
        P[3 + j] = tp[2] * Q[j] - tp[0] * Q[6 + j];
        P[6 + j] = tp[0] * Q[3 + j] - tp[1] * Q[j];
    }
    MISLAM_PG_UNROLL
    for (int i = 0; i < 3; i++) {
        MISLAM_PG_UNROLL
        for (int j = 0; j < 3; j++) {
            A[6 * i + j] = Q[3 * i + j];
            A[6 * i + 3 + j] = 0.0;
            A[6 * (3 + i) + j] = P[3 * i + j];
            A[6 * (3 + i) + 3 + j] = Q[3 * i + j];
        }
    }
}

// the weight of an edge and its share of the cost
MISLAM_PG_HD inline void pg_line_process(double chi2, bool uncertain, double mu, double* w, double* share)
{
    if (uncertain && mu > 0.0) {
        const double q = mu / (mu + chi2);
        *w = q * q;
        *share = (mu * chi2) / (mu + chi2);
    } else {
        *w = 1.0;
        *share = chi2;
    }
}

// r, chi2, w and share always; M and h only with want_system (the candidate pass of the outer loop asks for the cost alone)
MISLAM_PG_HD inline void pg_edge_terms(const double (&Ts)[PG_POSE], const double (&Tt)[PG_POSE], const double (&Z)[PG_POSE], const double (&L21)[PG_TRI],
                                       bool uncertain, double mu, bool want_system, double (&r)[6], double* chi2, double* w, double* share,
                                       double (&M21)[PG_TRI], double (&h)[6])
{
    double Rs[9], ts[3], Rt[9], tt[3], Rz[9], tz[3];
    MISLAM_PG_UNROLL
    for (int i = 0; i < 9; i++) { Rs[i] = Ts[i]; Rt[i] = Tt[i]; Rz[i] = Z[i]; }
    MISLAM_PG_UNROLL
    for (int i = 0; i < 3; i++) { ts[i] = Ts[9 + i]; tt[i] = Tt[9 + i]; tz[i] = Z[9 + i]; }
    double Ri[9], ti[3], Rzi[9], tzi[3], Ra[9], ta[3], Re[9], te[3];
    pg_inverse(Rt, tt, Ri, ti);
    pg_inverse(Rz, tz, Rzi, tzi);
    pg_product(Ri, ti, Rs, ts, Ra, ta);
    pg_product(Ra, ta, Rzi, tzi, Re, te);
    double om[3];
    pg_log_so3(Re, om);
    MISLAM_PG_UNROLL
    for (int i = 0; i < 3; i++) { r[i] = om[i]; r[3 + i] = te[i]; }

    double L[36];
    {
        int k = 0;
        MISLAM_PG_UNROLL
        for (int i = 0; i < 6; i++) {
            MISLAM_PG_UNROLL
            for (int j = i; j < 6; j++) { L[6 * i + j] = L21[k]; L[6 * j + i] = L21[k]; k++; }
        }
    }
    double u[6];
    MISLAM_PG_UNROLL
    for (int i = 0; i < 6; i++) {
        double s = 0.0;
        MISLAM_PG_UNROLL
        for (int j = 0; j < 6; j++) s += L[6 * i + j] * r[j];
        u[i] = s;
    }
    double c2 = 0.0;
    MISLAM_PG_UNROLL
    for (int i = 0; i < 6; i++) c2 += r[i] * u[i];
    *chi2 = c2;
    pg_line_process(c2, uncertain, mu, w, share);
    if (!want_system) return;

    double A[36];
    pg_adjoint(Rt, tt, A);
    // B = Lambda A, then M = w A^T B (its upper triangle) and h = w A^T u
    double B[36];
    MISLAM_PG_UNROLL
    for (int i = 0; i < 6; i++) {
        MISLAM_PG_UNROLL
        for (int j = 0; j < 6; j++) {
            double s = 0.0;
            MISLAM_PG_UNROLL
            for (int k = 0; k < 6; k++) s += L[6 * i + k] * A[6 * k + j];
            B[6 * i + j] = s;
        }
    }
    const double ww = *w;
    {
        int k = 0;
        MISLAM_PG_UNROLL
        for (int i = 0; i < 6; i++) {
            MISLAM_PG_UNROLL
            for (int j = i; j < 6; j++) {
                double s = 0.0;
                MISLAM_PG_UNROLL
                for (int q = 0; q < 6; q++) s += A[6 * q + i] * B[6 * q + j];
                M21[k++] = ww * s;
            }
        }
    }
    MISLAM_PG_UNROLL
    for (int i = 0; i < 6; i++) {
        double s = 0.0;
        MISLAM_PG_UNROLL
        for (int q = 0; q < 6; q++) s += A[6 * q + i] * u[q];
        h[i] = ww * s;
    }
}

// y = M d for a symmetric M given by its upper triangle: y_i = sum_j M_ij d_j, j ascending from 0
MISLAM_PG_HD inline void pg_sym_apply(const double (&M21)[PG_TRI], const double (&d)[6], double (&y)[6])
{
    double M[36];
    {
        int k = 0;
        MISLAM_PG_UNROLL
        for (int i = 0; i < 6; i++) {
            MISLAM_PG_UNROLL
            for (int j = i; j < 6; j++) { M[6 * i + j] = M21[k]; M[6 * j + i] = M21[k]; k++; }
        }
    }
    MISLAM_PG_UNROLL
    for (int i = 0; i < 6; i++) {
        double s = 0.0;
        MISLAM_PG_UNROLL
        for (int j = 0; j < 6; j++) s += M[6 * i + j] * d[j];
        y[i] = s;
    }
}

// the index of the diagonal entry (i, i) in the 21 numbers of an upper triangle
MISLAM_PG_HD inline int pg_tri_diag(int i) { return i * 6 - (i * (i - 1)) / 2; }

// A list entry is 2 * edge + side (side 0: the node is the edge's source, 1: its target); a node's list ascends in it.
MISLAM_PG_HD inline int pg_list_slot(int edge, int side) { return 2 * edge + side; }

}  // namespace mislam
