"""A float64 reference of what lies between the CPD E-step's per-point outputs and the next transform: the M-step's 19 moments, the
one-lane solve (MStep, coherentpointdrift.cpp:223-277), the exact sigma^2_0 and the transform of the moving cloud.  numpy only.  Shared
by tests/test_mstep_reference.py (CPU: against the oracle's M-step on the bunny fixture) and tests/test_gpu_cpd_moments.py (every route
that produces the moments on the device).

  moments(b, a, p1, pt1, px)   the 18 sums that are functions of the arrays alone, and per sum the sum of its terms' absolute values:
                               xs[1..3] = sum pt1 a_d, xs[4] = sum pt1 |a|^2, ks[0] = sum p1, ks[1..3] = sum p1 b_d,
                               ks[4 + 3r + c] = sum b_r px_c, ks[13] = sum p1 |b|^2        (xs[0], the sum of log den, is no function of them)
  solve(xs, ks, const_scale, scale_in)   the M-step from the moments, every operation in float64
  sigma2_exact(b, a)           sum_ij |a_i - b_j|^2 / (3 m n) from centred sums (no cancellation of its own)
  transform(b, R, t, s)        s*((R0*x + R3*y) + R6*z) + t in float32, operation by operation as cpd_transform_point (cpd_math.hpp)

Every product of two float32 values is exact in float64 (24 + 24 bits), so a term of a moment is exact; the sums are taken in extended
precision (np.longdouble, pairwise) and rounded once: the reference's own error is below 2^-60 of the sum of the absolute terms."""
import numpy as np

U64 = 2.0 ** -53
U32 = 2.0 ** -24
XS_ARRAY_SUMS = (1, 2, 3, 4)                  # indices of xs that moments() determines
KS_SUMS = tuple(range(14))


def _sum(v):
    return float(np.sum(np.asarray(v, np.longdouble)))


def moments(b, a, p1, pt1, px):
    """-> (xs[5], ks[14], xs_abs[5], ks_abs[14]) in float64; xs[0] and xs_abs[0] are NaN (not determined by the arrays)."""
    b = np.asarray(b, np.float32).astype(np.longdouble).reshape(-1, 3)
    a = np.asarray(a, np.float32).astype(np.longdouble).reshape(-1, 3)
    p1 = np.asarray(p1, np.float32).astype(np.longdouble).ravel()
    pt1 = np.asarray(pt1, np.float32).astype(np.longdouble).ravel()
    px = np.asarray(px, np.float32).astype(np.longdouble).reshape(-1, 3)
    assert len(b) == len(p1) == len(px) and len(a) == len(pt1)
    xs, ks = np.full(5, np.nan), np.zeros(14)
    xs_abs, ks_abs = np.full(5, np.nan), np.zeros(14)

    def put(dst, dst_abs, i, terms):
        dst[i], dst_abs[i] = _sum(terms), _sum(np.abs(terms))

    for d in range(3):
        put(xs, xs_abs, 1 + d, a[:, d] * pt1)
        put(ks, ks_abs, 1 + d, b[:, d] * p1)
    put(xs, xs_abs, 4, (a * a).sum(axis=1) * pt1)
    put(ks, ks_abs, 0, p1)
    for r in range(3):
        for c in range(3):
            put(ks, ks_abs, 4 + 3 * r + c, b[:, r] * px[:, c])
    put(ks, ks_abs, 13, (b * b).sum(axis=1) * p1)
    return xs, ks, xs_abs, ks_abs


def solve(xs, ks, const_scale, scale_in=1.0):
    """MStep (coherentpointdrift.cpp:223-277) from the reduced moments, in float64.  numpy's SVD; the rotation is U diag(1, 1, det(U V^T)) V^T and
    the scale's numerator (S0 + S1) + S2 det(U V^T), the determinant rule of the device's solve (svd3.hpp kabsch_rotation, cpd_math.hpp).
    -> dict(R [3,3] row-major, t, scale, sigma2, Np, sigmaSubtrahend, scaleDenominator, scaleNumerator, ca, cb, S)."""
    xs, ks = np.asarray(xs, np.float64), np.asarray(ks, np.float64)
    Np = ks[0]
    inv = 1.0 / Np
    cb, ca = inv * ks[1:4], inv * xs[1:4]                       # centerBefore, centerAfter
    # AMatrix = (EigenBefore * px)^T - Np * centerAfter * centerBefore^T;  (EigenBefore * px)[r][c] = ks[4 + 3r + c]
    A = ks[4:13].reshape(3, 3).T - Np * np.outer(ca, cb)
    Um, S, Vt = np.linalg.svd(A)
    det = float(np.linalg.det(Um @ Vt))
    R = Um @ np.diag([1.0, 1.0, det]) @ Vt
    num = (S[0] + S[1]) + S[2] * det
    sub = xs[4] - Np * float(ca @ ca)
    den = ks[13] - Np * float(cb @ cb)
    if const_scale:
        scale = float(scale_in)
        sigma2 = inv * abs(sub + den - 2.0 * num) / 3.0
    else:
        scale = num / den
        sigma2 = inv * abs(sub - scale * num) / 3.0
    t = ca - scale * (R @ cb)
    return dict(R=R, t=t, scale=scale, sigma2=sigma2, Np=Np, sigmaSubtrahend=sub, scaleDenominator=den, scaleNumerator=num, ca=ca, cb=cb, S=S)


def sigma2_exact(b, a):
    """sum_ij |a_i - b_j|^2 / (3 m n) = (sum_j |b_j - cb|^2 / m + sum_i |a_i - ca|^2 / n + |ca - cb|^2) / 3 -- every term non-negative: no
    cancellation, whatever the clouds' offset.  Extended precision throughout."""
    b = np.asarray(b, np.float32).astype(np.longdouble).reshape(-1, 3)
    a = np.asarray(a, np.float32).astype(np.longdouble).reshape(-1, 3)
    cb, ca = b.sum(axis=0) / len(b), a.sum(axis=0) / len(a)
    vb = np.sum((b - cb) ** 2) / len(b)
    va = np.sum((a - ca) ** 2) / len(a)
    return float((vb + va + np.sum((ca - cb) ** 2)) / 3)


def transform(b, R, t, s):
    """y = s * ((R[:,0] x + R[:,1] y) + R[:,2] z) + t in float32, one rounding per operation, in cpd_transform_point's order.  R [3,3] row-major
    (R[i][j] = the state's R[3 j + i])."""
    b = np.asarray(b, np.float32).reshape(-1, 3)
    R, t, s = np.asarray(R, np.float32), np.asarray(t, np.float32), np.float32(s)
    x, y, z = b[:, 0], b[:, 1], b[:, 2]
    out = np.empty_like(b)
    for i in range(3):
        out[:, i] = s * ((R[i, 0] * x + R[i, 1] * y) + R[i, 2] * z) + t[i]
    return out


# ---- the device's accumulation orders (cpd_kernels.hip, cpd_trunc.hip, cpd_fgt.hip, reduce.hpp), for the bound of a moment ----
SUM_ROWS_CAP, TRUNC_ROWS_CAP = 512, 4096          # ICP_MAX_PARTIAL_BLOCKS, CPD_TRUNC_MAX_BLOCKS
POINTS_PER_ROW = {"post": 64, "trunc": 64, "standalone": 256}


def sum_rows(points, producer):
    """Rows of fp64 partial sums the producer leaves for `points` points (cpd_sum_blocks, cpd_standalone_sum_blocks, the truncated tiles)."""
    cap = TRUNC_ROWS_CAP if producer == "trunc" else SUM_ROWS_CAP
    per = POINTS_PER_ROW[producer]
    return max(1, min(cap, (points + per - 1) // per))


def additions(points, producer, width):
    """The longest chain of fp64 additions a term of a moment goes through.  A lane adds one term per grid-stride trip, ceil(groups / rows)
    trips (groups = ceil(points / points per row)); the lanes of a wave are added by a shuffle tree of 6 levels (reduce.hpp wave_sum); the
    post kernels, the stand-alone kernels and the FGT's post kernels add the four waves' sums in order (block_sum_store: 3 -- the truncated
    kernels keep the sums on wave 0: none); the rows are summed by one workgroup (reduce_partials), 256 / width row groups of
    ceil(rows / groups) rows in order, then the groups in order.  width: 8 for the x-sums, 16 for the k-sums."""
    per = POINTS_PER_ROW[producer]
    rows = sum_rows(points, producer)
    groups = (points + per - 1) // per
    trips = (groups + rows - 1) // rows
    in_block = 6 + (0 if producer == "trunc" else 3)
    g = 256 // width
    return trips + in_block + (rows + g - 1) // g + g


def moment_bounds(m, n, producer, xs_abs, ks_abs):
    """|device - reference| allowed per moment: gamma_k sum|term| with k = additions(...) -- any order of k additions per term has at most
    that error -- and for xs[4] / ks[13], whose squares a_d a_d / b_d b_d are rounded to float32 before the (exact) product with the weight
    and whose three products are added first (2 more additions), + 2^-24 sum|term|.  A sum whose terms are all zero has bound 0."""
    def gamma(k):
        return k * U64 / (1.0 - k * U64)
    kx, kk = additions(n, producer, 8), additions(m, producer, 16)
    bx = np.array([np.nan] + [gamma(kx) * xs_abs[i] for i in (1, 2, 3)] + [(gamma(kx + 2) + U32) * xs_abs[4]])
    bk = np.array([gamma(kk) * ks_abs[i] for i in range(13)] + [(gamma(kk + 2) + U32) * ks_abs[13]])
    return bx, bk


# ---- sigma^2 out of the solve: the fp32 operations between the moments and it (cpd_math.hpp cpd_solve_body, svd3.hpp) ----
# Centres: Np narrowed (1), 1 / Np (1), the product narrowed (1): 3 u each.  sigmaSubtrahend = (float) xs[4] - Np |ca|^2: the narrowing (1), and
# on Np |ca|^2 -- which for a cloud centred at the origin is below the first term -- squares 2 * 3 + 1, two additions, Np (1), the product (1): 11,
# the subtraction (1): at most 13 u |sigmaSubtrahend| + ... <= C_CENTRED u (|xs[4]| + Np |ca|^2).  scaleDenominator likewise.
# scaleNumerator = (S0 + S1) + S2 det: the singular values of the two-sided Jacobi sweeps.  An error of a rotation's ANGLE costs nothing (the
# sweeps converge on whatever orthogonal factors they apply); what moves the singular values is each applied rotation's departure from
# orthogonality and the rounding of its application: c^2 + s^2 of the right rotation is off by <= 6 u (t^2 + 1: 2, the root's reciprocal: 2,
# s = t n: 1, squared), of the left one -- a product of two such -- by <= 18 u; applying one costs 3 u (two products, one addition) per entry:
# a row and a column rotation per pair change an entry's norm by <= (9 + 3) + (3 + 3) = 18 u, a diagonal entry is in two of a sweep's three
# pairs: 36 u per sweep; at most 5 rotating sweeps (quadratic convergence; the cap is 64), the scaling by 1 / max|A| and back (3), the
# off-diagonal residue the stopping threshold leaves (2 FLT_EPSILON max diag per entry: 8 u by Weyl): 191 u max(S) per singular value.  The
# determinant carries U's and V's departure from orthogonality (another 190 u) on S2; three values and two additions: <= 770 u numerator,
# 800 with the narrowing of A's entries and the centres' product in them (2 + 10 u of entries no larger than max(S)).
C_CENTRED, C_NUMERATOR = 16.0, 800.0


def sigma2_bound(sol, const_scale):
    """Absolute bound of |device sigma^2 - solve()'s|: scale-free sigma^2 = |sub - s num| / (3 Np), s = num / den: d(s num) / (s num) = 2 dnum/num
    + dden/den + 2 u (the quotient, the product), the subtraction, 1 / Np (2), the product with it and the division by 3 (2):
    c = 2 C_NUMERATOR + 2 C_CENTRED + 8 on (|sub| + |s num|); constant scale |sub + den - 2 num|: the same c on the three terms."""
    c = 2 * C_NUMERATOR + 2 * C_CENTRED + 8
    sub, den, num = abs(sol["sigmaSubtrahend"]), abs(sol["scaleDenominator"]), abs(sol["scaleNumerator"])
    if const_scale:
        mag = sub + den + 2 * num
    else:
        mag = sub + abs(sol["scale"]) * num
    return c * U32 * mag / (3.0 * abs(sol["Np"]))


def sigma2_init_bound(b, a):
    """Relative bound of the device's exact sigma^2_0 (cpd_init_sums_kernel, cpd_init_state_body): eight fp64 sums over at most max(m, n) points
    (gamma_k on sums of non-negative squares, on the coordinate sums relative to sum |x|), then N sum|b|^2 + M sum|a|^2 - 2 sum a . sum b in
    fp64 -- eight more roundings on terms that are `cancel` times the result, cancel = (the three terms' magnitudes) / result ~ (offset /
    extent)^2 -- and one narrowing to float32.  k: the init kernel is grid-stride over 256-point rows with the 512-row cap, one workgroup sums
    the rows (width 8)."""
    b64 = np.asarray(b, np.float32).astype(np.float64).reshape(-1, 3)
    a64 = np.asarray(a, np.float32).astype(np.float64).reshape(-1, 3)
    m, n = len(b64), len(a64)
    k = additions(max(m, n), "standalone", 8) + 2
    # magnitudes of the three terms with the coordinate sums taken absolutely: what an error of gamma_k per sum can move
    terms = n * (b64 ** 2).sum() + m * (a64 ** 2).sum() + 2.0 * (np.abs(a64).sum(axis=0) * np.abs(b64).sum(axis=0)).sum()
    result = 3.0 * m * n * sigma2_exact(b, a)
    cancel = terms / result
    return (2 * k + 8) * U64 * cancel + U32
