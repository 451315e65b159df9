"""The restatement mi_mls_smooth is tested against (numpy float64, CPU), built on tests/knn_reference.py, as include/mi_slam.h states the
rules:

  ball       r2 = float32(radius) * float32(radius); { j : d2(q, j) <= r2 } with d2 the float32 matrix of knn_reference.d2_matrix in the
             arithmetic of dist_mode; nothing is skipped, so in self mode point i is in its own ball
  plane      d = float64(p_j) - float64(q); S = sum d, Q = sum d d^T; c = |ball|; m = S / c; C = Q / c - m m^T; numpy.linalg.eigh(C):
             lambda ascending, n the normalised eigenvector of lambda0 (numpy's sign); curvature = max(lambda0, 0) / trace, 0 where the trace
             is not positive; o = ((n . m)) n
  frame      k = argmin |n_k| (the lowest on ties); u = (e_k x n) / |e_k x n|; v = n x u
  quadratic  order == 2 and c >= 6: e = d - o; a = u . e, b = v . e, f = n . e; w = exp(-(d . d) / s^2); phi = (1, a, b, aa, ab, bb);
             A = sum w phi phi^T, g = sum w phi f; A x = g by solve6 below: plane_solve.hpp's plane_solve6, operation for operation, over
             all queries at once
  outputs    status 0: (q + o) + x0 n and normalise((n - x1 u) - x2 v); status 1: q + o and n; status 2 (c < min_neighbours): q's bits,
             a zero normal, curvature 0

Every sum runs over the ball in ASCENDING index order (`descending=True`: the other way round), one addition after the other
(numpy.cumsum; a point outside the ball adds an exact 0).  The device sums in its walk's order: the GPU tests' bound covers the difference.
`pivot` is the smallest pivot of the restatement's own scaled LDL^T (0 where a diagonal entry was unusable or the solve did not run)."""
import numpy as np

import knn_reference as K

PIVOT_MIN = 1e-10                 # PLANE_PIVOT_MIN
QUADRATIC_MIN = 6                 # MLS_QUADRATIC_MIN
QUADRATIC, PLANE, UNTOUCHED = 0, 1, 2


def _seq(terms, descending):
    """the sum along axis 1, one addition after the other in index order"""
    if descending:
        terms = terms[:, ::-1]
    return np.cumsum(terms, axis=1)[:, -1]


def _dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def frame(n, rotation=0.0):
    """(u, v) of unit normals n [rows, 3]; rotation: the frame turned about n by that angle (the outputs must not care)"""
    k = np.argmin(np.abs(n), axis=1)
    x = np.cross(np.eye(3)[k], n)
    u = x / np.sqrt(_dot3(x, x))[:, None]
    v = np.cross(n, u)
    if rotation != 0.0:
        u = np.cos(rotation) * u + np.sin(rotation) * v
        v = np.cross(n, u)
    return u, v


def solve6(A, g):
    """(x [rows, 6], ok [rows], smallest pivot [rows]) of A x = g for A [rows, 6, 6] symmetric: the system scaled to a unit diagonal, LDL^T
    without pivoting, a diagonal entry that is not positive and finite or a pivot below PIVOT_MIN is degenerate (x = 0 there)."""
    rows = len(A)
    d = A[:, np.arange(6), np.arange(6)]
    with np.errstate(all="ignore"):
        good = (np.isfinite(d) & (d > 0)).all(axis=1)
        w = 1.0 / np.sqrt(np.where(d > 0, d, 1.0))
        S = (A * w[:, :, None]) * w[:, None, :]
        S[:, np.arange(6), np.arange(6)] = 1.0
        L, piv = np.zeros((rows, 6, 6)), np.zeros((rows, 6))
        smallest, usable = np.ones(rows), good.copy()
        for j in range(6):
            dj = S[:, j, j].copy()
            for k in range(j):
                dj = dj - (L[:, j, k] * L[:, j, k]) * piv[:, k]
            piv[:, j] = dj
            smallest = np.where(dj >= smallest, smallest, dj)
            usable &= dj >= PIVOT_MIN
            for i in range(j + 1, 6):
                s = S[:, i, j].copy()
                for k in range(j):
                    s = s - (L[:, i, k] * L[:, j, k]) * piv[:, k]
                L[:, i, j] = s / dj
        y = np.zeros((rows, 6))
        for i in range(6):
            s = g[:, i] * w[:, i]
            for k in range(i):
                s = s - L[:, i, k] * y[:, k]
            y[:, i] = s
        y = y / piv
        for i in range(5, -1, -1):
            s = y[:, i].copy()
            for k in range(i + 1, 6):
                s = s - L[:, k, i] * y[:, k]
            y[:, i] = s
        x = y * w
    smallest = np.where(good, smallest, 0.0)
    return np.where(usable[:, None], x, 0.0), usable, smallest


def conditioning(ref, radius):
    """What turns the rounding of a query's sums into the error of its projection, per query: where the quadratic was solved, the smallest
    pivot of the scaled system; where the plane alone answered, (lambda1 - lambda0) / radius^2, at most 1 -- the gap that holds the normal
    against a perturbation of the covariance, in the units of the sums' bound (the foot o = (n . m) n turns with n, |m| <= radius);
    1 for an untouched query."""
    r = float(np.float32(radius))
    gap = np.clip((ref["lam"][:, 1] - ref["lam"][:, 0]) / (r * r), 0.0, 1.0)
    return np.where(ref["status"] == QUADRATIC, ref["pivot"], np.where(ref["status"] == PLANE, gap, 1.0))


def error_unit(ref, radius):
    """(c + 8) 2^-53 radius / conditioning per query: the GPU tests' bound on a coordinate at K = 1 (tests/test_gpu_mls.py)"""
    with np.errstate(divide="ignore"):
        return (ref["neighbours"] + 8.0) * 2.0 ** -53 * float(np.float32(radius)) / conditioning(ref, radius)


def smooth(cloud, radius, dist_mode, queries=None, gauss_scale=0.0, order=2, min_neighbours=3, block=128, only=None, descending=False, frame_rotation=0.0):
    """dict of per-query results (of the queries `only` alone where given -- what a large case can afford):
    xyz, normals float32 [nq, 3]; curvature float32 [nq]; neighbours int32 [nq]; status uint8 [nq]; xyz64, normals64 float64 [nq, 3]: the
    same before the one rounding; lam float64 [nq, 3]; pivot float64 [nq]; plane_normal float64 [nq, 3]: n of the first stage."""
    cloud = np.ascontiguousarray(cloud, np.float32)
    Q = cloud if queries is None else np.ascontiguousarray(queries, np.float32)
    if only is not None:
        Q = Q[np.asarray(only, np.int64)]
    c64 = cloud.astype(np.float64)
    r2 = np.float32(radius) * np.float32(radius)
    s = np.float64(np.float32(gauss_scale)) if np.float32(gauss_scale) > 0 else np.float64(np.float32(radius))
    s2 = s * s
    nq = len(Q)
    out = {"xyz": Q.copy(), "normals": np.zeros((nq, 3), np.float32), "curvature": np.zeros(nq, np.float32), "neighbours": np.zeros(nq, np.int32),
           "status": np.full(nq, UNTOUCHED, np.uint8), "xyz64": Q.astype(np.float64), "normals64": np.zeros((nq, 3)), "lam": np.zeros((nq, 3)),
           "pivot": np.zeros(nq), "plane_normal": np.zeros((nq, 3))}
    for lo in range(0, nq, block):
        q = Q[lo:lo + block]
        inside = K.d2_matrix(q, cloud, dist_mode) <= r2
        cols = np.flatnonzero(inside.any(axis=0))                      # (ascending: the order among the ball's points is kept)
        inside = inside[:, cols]
        count = inside.sum(axis=1)
        out["neighbours"][lo:lo + len(q)] = count
        fit = np.flatnonzero(count >= min_neighbours)
        if len(fit) == 0:
            continue
        inside, c = inside[fit], count[fit].astype(np.float64)
        q64 = q[fit].astype(np.float64)
        d = (c64[cols][None, :, :] - q64[:, None, :]) * inside[:, :, None]              # (0 outside the ball)
        S = np.stack([_seq(d[:, :, a], descending) for a in range(3)], axis=1)
        pairs = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
        Qs = [_seq(d[:, :, a] * d[:, :, b], descending) for a, b in pairs]
        m = S / c[:, None]
        cov = np.zeros((len(fit), 3, 3))
        for (a, b), qab in zip(pairs, Qs):
            cov[:, a, b] = cov[:, b, a] = qab / c - m[:, a] * m[:, b]
        lam, vec = np.linalg.eigh(cov)
        n = vec[:, :, 0]
        n = n / np.sqrt(_dot3(n, n))[:, None]
        trace = (lam[:, 0] + lam[:, 1]) + lam[:, 2]
        with np.errstate(divide="ignore", invalid="ignore"):
            curv = np.where(trace > 0, np.maximum(lam[:, 0], 0.0) / trace, 0.0)
        o = _dot3(n, m)[:, None] * n
        u, v = frame(n, frame_rotation)

        xyz, normal, status, pivot = q64 + o, n.copy(), np.full(len(fit), PLANE, np.uint8), np.zeros(len(fit))
        quad = np.flatnonzero(c >= QUADRATIC_MIN) if order == 2 else np.zeros(0, np.int64)
        if len(quad):
            dq, w_in = d[quad], inside[quad]
            e = dq - o[quad][:, None, :]
            a_ = _dot3(u[quad][:, None, :], e)
            b_ = _dot3(v[quad][:, None, :], e)
            f_ = _dot3(n[quad][:, None, :], e)
            w = np.exp(-(_dot3(dq, dq) / s2)) * w_in
            phi = [np.ones_like(a_), a_, b_, a_ * a_, a_ * b_, b_ * b_]
            A, g = np.zeros((len(quad), 6, 6)), np.zeros((len(quad), 6))
            for i in range(6):
                wp = w * phi[i]
                for j in range(i, 6):
                    A[:, i, j] = A[:, j, i] = _seq(wp * phi[j], descending)
                g[:, i] = _seq(wp * f_, descending)
            x, ok, smallest = solve6(A, g)
            pivot[quad] = smallest
            good = quad[ok]
            xg = x[ok]
            xyz[good] = (q64[good] + o[good]) + xg[:, 0:1] * n[good]
            mm = (n[good] - xg[:, 1:2] * u[good]) - xg[:, 2:3] * v[good]
            normal[good] = mm / np.sqrt(_dot3(mm, mm))[:, None]
            status[good] = QUADRATIC
        rows = lo + fit
        out["xyz64"][rows], out["normals64"][rows], out["status"][rows], out["pivot"][rows] = xyz, normal, status, pivot
        out["xyz"][rows], out["normals"][rows], out["curvature"][rows] = xyz.astype(np.float32), normal.astype(np.float32), curv.astype(np.float32)
        out["lam"][rows], out["plane_normal"][rows] = lam, n
    return out
