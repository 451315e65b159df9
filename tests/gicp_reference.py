"""The restatement mi_estimate_covariances, mi_icp_gicp_register and mi_gicp_system are tested against (numpy, CPU): the rules of
include/mi_slam.h retraced one by one, in the header's order of operations, vectorised over the points.  Built on tests/knn_reference.py
(the keys), tests/normals_reference.py (the eigenvector of MI_COV_PLANE) and tests/plane_reference.py (the fp32 move, the centre, the
solve, Rodrigues' formula, the composition: generalized ICP shares them with the point-to-plane registration).

Covariances here are [points, 6] arrays, the upper triangle row by row: xx, xy, xz, yy, yz, zz.  Matrices are indexed [row, col]."""
import numpy as np

import knn_reference as K
import plane_reference as P

COV_RAW, COV_PLANE = 0, 1
STOP_CONVERGED, STOP_MAX_ITERATIONS, STOP_NO_PAIRS, STOP_DEGENERATE = P.STOP_CONVERGED, P.STOP_MAX_ITERATIONS, P.STOP_NO_PAIRS, P.STOP_DEGENERATE
TRI = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))


def sym(c6, i, k):
    """entry (i, k) of symmetric matrices held as [..., 6]"""
    lo, hi = min(i, k), max(i, k)
    return c6[..., hi if lo == 0 else lo + hi + 1]


def full(c6):
    """[..., 3, 3] of [..., 6]"""
    c6 = np.asarray(c6)
    return np.stack([np.stack([sym(c6, i, k) for k in range(3)], axis=-1) for i in range(3)], axis=-2)


def plane_covariance(normal, epsilon):
    """I - (1 - epsilon) n n^T as [..., 6] float64, in the header's order: w = 1 - epsilon, u = w n, entry ab = delta_ab - u_a n_b"""
    n = np.asarray(normal, np.float64)
    w = 1.0 - np.float64(np.float32(epsilon))
    u = w * n
    return np.stack([(1.0 if a == b else 0.0) - u[..., a] * n[..., b] for a, b in TRI], axis=-1)


def one_pass_covariance(cloud, idx):
    """(C [n, 6] float64, count [n]) from the neighbour lists idx [n, k] in key order (-1: no neighbour in that slot): the nine running
    sums of the differences, added slot by slot, then m = S / c and C_ab = Q_ab / c - m_a m_b with c = count + 1"""
    p = np.ascontiguousarray(cloud, np.float32).astype(np.float64)
    n = len(p)
    S, Q, count = np.zeros((n, 3)), np.zeros((n, 6)), np.zeros(n, np.int32)
    for slot in range(idx.shape[1]):
        have = idx[:, slot] >= 0
        d = p[np.where(have, idx[:, slot], 0)] - p
        S = np.where(have[:, None], S + d, S)
        Q = np.where(have[:, None], Q + np.stack([d[:, a] * d[:, b] for a, b in TRI], axis=1), Q)
        count += have
    c = (count + 1).astype(np.float64)
    m = S / c[:, None]
    C = np.stack([Q[:, k] / c - m[:, a] * m[:, b] for k, (a, b) in enumerate(TRI)], axis=1)
    return C, count


def covariances(cloud, k, mode=COV_PLANE, epsilon=1e-3, dist_mode=K.DIST_CPU_ROUNDING, max_d2=np.inf, idx=None):
    """mi_estimate_covariances -> dict(cov float32 [n, 6], cov64: the same before its rounding, count int32 [n], C float64 [n, 6]: the
    neighbourhood's covariance, lam [n, 3]: its eigenvalues, ascending).  MI_COV_PLANE's eigenvector comes from numpy.linalg.eigh where the
    device runs a Jacobi iteration: the two agree as far as the eigen-gap lets them, which is what the tests' tolerance is for.
    idx: the neighbour lists, where the caller holds them already."""
    if idx is None:
        idx, _, _ = K.knn(None, cloud, k, dist_mode, max_d2)
    C, count = one_pass_covariance(cloud, idx)
    lam, V = np.linalg.eigh(full(C))
    out = C if mode == COV_RAW else plane_covariance(V[:, :, 0], epsilon)
    out = np.where((count >= 2)[:, None], out, 0.0)
    return dict(cov=out.astype(np.float32), cov64=out, count=count, C=C, lam=lam)


def inverse_sym3(S):
    """(M [..., 6], det [...]) of symmetric S [..., 6] by the adjugate over the determinant, in the header's order"""
    s00, s01, s02, s11, s12, s22 = (S[..., k] for k in range(6))
    c00, c01, c02 = s11 * s22 - s12 * s12, s02 * s12 - s01 * s22, s01 * s12 - s02 * s11
    c11, c12, c22 = s00 * s22 - s02 * s02, s01 * s02 - s00 * s12, s00 * s11 - s01 * s01
    det = (s00 * c00 + s01 * c01) + s02 * c02
    with np.errstate(all="ignore"):
        M = np.stack([c00, c01, c02, c11, c12, c22], axis=-1) / det[..., None]
    return M, det


def sigma(Rf, cov_a, cov_b):
    """Sigma [..., 6] = C_a + Rf C_b Rf^T in the header's order; Rf float64 [3, 3] (already rounded to fp32), the covariances float64"""
    T = [[(Rf[r, 0] * sym(cov_b, 0, c) + Rf[r, 1] * sym(cov_b, 1, c)) + Rf[r, 2] * sym(cov_b, 2, c) for c in range(3)] for r in range(3)]
    return np.stack([sym(cov_a, r, c) + ((T[r][0] * Rf[c, 0] + T[r][1] * Rf[c, 1]) + T[r][2] * Rf[c, 2]) for r, c in TRI], axis=-1)


def cross(p, y):
    """P x y, component by component: two products and one subtraction each"""
    return [p[1] * y[2] - p[2] * y[1], p[2] * y[0] - p[0] * y[2], p[0] * y[1] - p[1] * y[0]]


def pair_terms(M, p, d):
    """the 28 float64 terms of every pair, header order: 21 of H (upper triangle, row-major), 6 of g, e.  M [k, 6], p and d [k, 3]"""
    p, d = [p[:, i] for i in range(3)], [d[:, i] for i in range(3)]
    W = [[None] * 6 for _ in range(3)]
    for r in range(3):
        Mr = [sym(M, r, c) for c in range(3)]
        W[r][:3] = cross(p, Mr)
        W[r][3:] = Mr
    H = [[None] * 6 for _ in range(6)]
    for b in range(6):
        col = [W[0][b], W[1][b], W[2][b]]
        H[0][b], H[1][b], H[2][b] = cross(p, col)
        H[3][b], H[4][b], H[5][b] = col
    Md = [(sym(M, r, 0) * d[0] + sym(M, r, 1) * d[1]) + sym(M, r, 2) * d[2] for r in range(3)]
    g = cross(p, Md) + Md
    e = (d[0] * Md[0] + d[1] * Md[1]) + d[2] * Md[2]
    return [H[a][b] for a in range(6) for b in range(a, 6)] + g + [e]


def candidate_pairs(q, after, cov_b, cov_a, Rf, idx):
    """For the candidates (i, idx[i]) with idx[i] >= 0: (rows i, M [k, 6], det [k]).  The covariances are promoted as they come: the device's
    are float32, and a float64 array here is the same rule without that rounding (what tests/test_gicp_reference.py pins the algebra with)."""
    rows = np.flatnonzero(np.asarray(idx) >= 0)
    S = sigma(Rf, np.asarray(cov_a)[np.asarray(idx)[rows]].astype(np.float64), np.asarray(cov_b)[rows].astype(np.float64))
    M, det = inverse_sym3(S)
    return rows, M, det


def sums_of_pairs(q, after, cov_b, cov_a, R, idx, d2):
    """(sums float64 [32], the sums of the terms' magnitudes, idx with the pairs of a bad determinant taken out) of the candidates
    (i, idx[i]) with idx[i] >= 0, the moved points q and the matches' float32 distances d2 being given; R: the fp64 pose's rotation"""
    after = np.ascontiguousarray(after, np.float32)
    Rf = np.asarray(R, np.float64).astype(np.float32).astype(np.float64)
    rows, M, det = candidate_pairs(q, after, cov_b, cov_a, Rf, idx)
    ok = (det > 0) & np.isfinite(det)
    rows, M = rows[ok], M[ok]
    out_idx = np.full(len(q), -1, np.int32)
    out_idx[rows] = np.asarray(idx)[rows]
    c0 = P.centre(after).astype(np.float64)
    qd = q[rows].astype(np.float64)
    terms = pair_terms(M, qd - c0, qd - after[out_idx[rows]].astype(np.float64)) + [np.asarray(d2)[rows].astype(np.float64)]
    sums, mags = np.zeros(32), np.zeros(32)
    for k, term in enumerate(terms):
        sums[k], mags[k] = term.sum(), np.abs(term).sum()
    sums[29] = mags[29] = float(len(rows))
    return sums, mags, out_idx


def system(before, cov_b, after, cov_a, R=None, t=None, dist_mode=K.DIST_CPU_ROUNDING, max_d2=np.inf):
    """One linearisation at the pose (R, t) (None: the identity) -> dict(sums float64 [32], abs float64 [32]: the sums of the terms'
    magnitudes, idx int32 [n]: the fixed index of every pair or -1, centre float32 [3], q float32 [n, 3])."""
    R = np.eye(3) if R is None else R
    t = np.zeros(3) if t is None else t
    after = np.ascontiguousarray(after, np.float32)
    q = P.move_f32(R, t, before)
    keys = K.sorted_keys(q, after, dist_mode, max_d2, keep=1)
    j, d2, count = K.unpack(keys, 1)
    j, d2 = j[:, 0], d2[:, 0]
    cand = (count == 1) & np.isfinite(d2)
    sums, mags, idx = sums_of_pairs(q, after, cov_b, cov_a, R, np.where(cand, j, -1), d2)
    return dict(sums=sums, abs=mags, idx=idx, centre=P.centre(after), q=q)


def step(before, cov_b, after, cov_a, R, t, dist_mode=K.DIST_CPU_ROUNDING, max_d2=np.inf):
    """One iteration from the pose (R, t) -> dict(stop: None / STOP_NO_PAIRS / STOP_DEGENERATE, R, t: the pose behind it (unchanged on a
    stop), omega, v: the update's lengths, error: sum e / pairs, system: the linearisation, kappa: cond(S) or inf)."""
    sy = system(before, cov_b, after, cov_a, R, t, dist_mode, max_d2)
    sums = sy["sums"]
    out = dict(system=sy, R=np.array(R, np.float64), t=np.array(t, np.float64), omega=np.nan, v=np.nan, kappa=np.inf,
               error=np.float32(sums[27] / sums[29]) if sums[29] > 0 else np.float32(0))
    if sums[29] < P.MIN_PAIRS:
        return dict(out, stop=STOP_NO_PAIRS)
    A, g = P.unpack_system(sums)
    S, _ = P.scaled(A)
    if S is not None:
        out["kappa"] = float(np.linalg.cond(S))
    x, _ = P.solve6(A, g)
    if x is None:
        return dict(out, stop=STOP_DEGENERATE)
    Rn, tn = P.compose(P.rodrigues(x[:3]), x[3:], sy["centre"], out["R"], out["t"])
    return dict(out, stop=None, R=Rn, t=tn, omega=float(np.linalg.norm(x[:3])), v=float(np.linalg.norm(x[3:])))


def register(before, cov_b, after, cov_a, eps_rotation=1e-6, eps_translation=1e-6, max_iterations=50, max_d2=np.inf, dist_mode=K.DIST_CPU_ROUNDING,
             init=None):
    """The whole loop -> dict(R, t float64, iterations, error float32, stop, poses: the fp64 pose before every iteration and the last one,
    steps: every iteration's step())."""
    init = np.eye(4) if init is None else np.asarray(init, np.float32).astype(np.float64)
    R, t = init[:3, :3].copy(), init[:3, 3].copy()
    poses, steps, iterations, error, stop = [(R, t)], [], 0, np.float32(0), STOP_MAX_ITERATIONS
    while iterations < max_iterations:
        s = step(before, cov_b, after, cov_a, R, t, dist_mode, max_d2)
        steps.append(s)
        error = s["error"]
        if s["stop"] is not None:
            stop = s["stop"]
            break
        R, t = s["R"], s["t"]
        poses.append((R, t))
        iterations += 1
        if s["omega"] <= np.float64(np.float32(eps_rotation)) and s["v"] <= np.float64(np.float32(eps_translation)):
            stop = STOP_CONVERGED
            break
        stop = STOP_MAX_ITERATIONS
    return dict(R=R, t=t, iterations=iterations, error=error, stop=stop, poses=poses, steps=steps)
