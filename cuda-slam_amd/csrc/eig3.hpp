// K14 building block: eigenvalues and eigenvectors of a symmetric 3x3 matrix, usable from one GPU lane and from host code (the
// surface normal of mi_estimate_normals, normals_kernels.hip; tests/eig3_selftest.cpp compiles this header alone with a host compiler).
//
// Cyclic Jacobi (Golub & Van Loan 8.5; Rutishauser's update formulas): the matrix is scaled by its largest |a_ij|, then the pairs
// (0,1), (0,2), (1,2) are swept; each rotation annihilates one off-diagonal entry with t = sgn(tau) / (|tau| + sqrt(tau^2 + 1)),
// tau = (a_qq - a_pp) / (2 a_pq), the smaller root, |t| <= 1.  A rotation is skipped once |a_pq| <= 2^-70 of the largest entry, far
// below the 2^-53 a double resolves beside it: convergence is quadratic, so the last sweep that still rotates leaves off-diagonal
// entries of that size, and the eigenvectors of a pair that is 1e-3 of the trace apart come out to about 1e-13 rather than eps / gap.
// The iteration stops when a sweep rotates nothing and after EIG3_MAX_SWEEPS sweeps whatever happened (NaN input cannot spin; a
// symmetric 3x3 needs 4 to 7).  Every entry of the matrix and of V is a named scalar: no index is computed at run time, so the
// device code holds everything in registers (no scratch), as svd3.hpp does.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MISLAM_EIG3_HD __host__ __device__
#else
#define MISLAM_EIG3_HD
#endif

#include <cmath>

namespace mislam {

constexpr int EIG3_MAX_SWEEPS = 16;

// One Jacobi rotation in the (p, q) plane of the symmetric matrix, r the third index: a_pq -> 0.  (vkp, vkq): columns p and q of V.
// Returns false when a_pq is already negligible and nothing was done.
template <class T>
MISLAM_EIG3_HD inline bool eig3_rotate(T& app, T& aqq, T& apq, T& arp, T& arq, T& v0p, T& v0q, T& v1p, T& v1q, T& v2p, T& v2q)
{
    using std::fabs;
    using std::sqrt;
    const T tiny = (T)8.470329472543003e-22;          // 2^-70 (the matrix is scaled: its largest entry is 1)
    if (!(fabs(apq) > tiny)) return false;
    const T tau = (aqq - app) / ((T)2 * apq);         // (may overflow to +-inf: then t = 0 and the rotation is the identity)
    const T w = sqrt(tau * tau + (T)1);
    const T t = (tau >= (T)0 ? (T)1 : (T)-1) / (fabs(tau) + w);
    const T c = (T)1 / sqrt(t * t + (T)1), s = t * c;
    app -= t * apq;
    aqq += t * apq;
    apq = (T)0;
    const T xp = arp, xq = arq;
    arp = c * xp - s * xq;
    arq = s * xp + c * xq;
    const T a0 = v0p, b0 = v0q, a1 = v1p, b1 = v1q, a2 = v2p, b2 = v2q;
    v0p = c * a0 - s * b0; v0q = s * a0 + c * b0;
    v1p = c * a1 - s * b1; v1q = s * a1 + c * b1;
    v2p = c * a2 - s * b2; v2q = s * a2 + c * b2;
    return true;
}

// a = {a00, a01, a02, a11, a12, a22} (the upper triangle, row by row).  lambda ascending; v row-major, v[3 r + i] = component r of
// the unit eigenvector of lambda[i] (the eigenvectors are the columns).  The zero matrix gives lambda = 0, V = I.
template <class T>
MISLAM_EIG3_HD inline void eig3_symmetric(const T a[6], T lambda[3], T v[9])
{
    using std::fabs;
    T scale = fabs(a[0]);
    scale = fabs(a[1]) > scale ? fabs(a[1]) : scale;
    scale = fabs(a[2]) > scale ? fabs(a[2]) : scale;
    scale = fabs(a[3]) > scale ? fabs(a[3]) : scale;
    scale = fabs(a[4]) > scale ? fabs(a[4]) : scale;
    scale = fabs(a[5]) > scale ? fabs(a[5]) : scale;
    const T div = scale > (T)0 ? scale : (T)1;
    T a00 = a[0] / div, a01 = a[1] / div, a02 = a[2] / div, a11 = a[3] / div, a12 = a[4] / div, a22 = a[5] / div;
    T v00 = 1, v01 = 0, v02 = 0, v10 = 0, v11 = 1, v12 = 0, v20 = 0, v21 = 0, v22 = 1;

    for (int sweep = 0; sweep < EIG3_MAX_SWEEPS; sweep++) {
        bool rotated = eig3_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);      // (p, q, r) = (0, 1, 2)
        rotated |= eig3_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);          // (0, 2, 1)
        rotated |= eig3_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);          // (1, 2, 0)
        if (!rotated) break;
    }

    // ascending, by three compare-and-swaps with static indices (a position computed at run time would put V into scratch)
    T l0 = a00 * scale, l1 = a11 * scale, l2 = a22 * scale;
#define MISLAM_EIG3_SWAP(la, lb, xa, xb, ya, yb, za, zb)                                  \
    {                                                                                     \
        const bool sw = lb < la;                                                          \
        const T tl = la, tx = xa, ty = ya, tz = za;                                       \
        la = sw ? lb : tl; lb = sw ? tl : lb;                                             \
        xa = sw ? xb : tx; xb = sw ? tx : xb;                                             \
        ya = sw ? yb : ty; yb = sw ? ty : yb;                                             \
        za = sw ? zb : tz; zb = sw ? tz : zb;                                             \
    }
    MISLAM_EIG3_SWAP(l0, l1, v00, v01, v10, v11, v20, v21)
    MISLAM_EIG3_SWAP(l1, l2, v01, v02, v11, v12, v21, v22)
    MISLAM_EIG3_SWAP(l0, l1, v00, v01, v10, v11, v20, v21)
#undef MISLAM_EIG3_SWAP
    lambda[0] = l0; lambda[1] = l1; lambda[2] = l2;
    v[0] = v00; v[1] = v01; v[2] = v02;
    v[3] = v10; v[4] = v11; v[5] = v12;
    v[6] = v20; v[7] = v21; v[8] = v22;
}

}  // namespace mislam
