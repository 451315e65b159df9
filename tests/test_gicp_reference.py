"""CPU suite: the restatement the GPU tests of generalized ICP use as their oracle (tests/gicp_reference.py), pinned in float64 against
independent forms of the same algebra.

  plane limit     With C_b = 0 and C_a = (I + kappa n n^T)^-1, kappa = 1 / eps - 1, the information matrix is M = I + kappa n n^T, and every
                  pair's H, g and e are the point-to-point terms J^T J, J^T d, d^T d plus kappa times the point-to-plane terms of
                  tests/plane_reference.py.  For a unit normal C_a is I - (1 - eps) n n^T; the scene's normals are float32 and off unit
                  length by 1e-7, so C_a is formed by Sherman-Morrison from the normal as it is, which keeps M's form exact.  The two sides
                  associate differently and the adjugate inverse of C_a, cond(C_a) = 1 / eps, carries cond 2^-53:
                  | difference | <= 64 * 2^-53 * (1 / eps) * sum |term|, sum |term| being that of the point-to-point terms plus that of the
                  unscaled plane terms, at eps = 1e-2.
  point to point  With C_a = I and C_b = 0 a step is the Gauss-Newton point-to-point step: numpy.linalg.solve of sum J^T J x = -sum J^T d.
  inverse         the adjugate inverse against numpy.linalg.inv to 1e-12 cond.
  covariances     MI_COV_PLANE has the eigenvalues (eps, 1, 1) to 1e-12; MI_COV_RAW is the two-pass covariance of tests/normals_reference.py
                  to a few 2^-53 of the trace."""
import numpy as np

import gicp_reference as G
import knn_reference as K
import normals_reference as N
import plane_reference as P
from test_gpu_plane import LIMIT, scene

EPS = 1e-2


def jacobians(p):
    """J = [ -[P]x , I ] per pair, [k, 3, 6]"""
    J = np.zeros((len(p), 3, 6))
    J[:, 0, 1], J[:, 0, 2] = p[:, 2], -p[:, 1]
    J[:, 1, 0], J[:, 1, 2] = -p[:, 2], p[:, 0]
    J[:, 2, 0], J[:, 2, 1] = p[:, 1], -p[:, 0]
    J[:, :, 3:] = np.eye(3)
    return J


def point_to_point_terms(q, after, idx):
    """(sums [28], sums of magnitudes [28]) of J^T J (upper triangle), J^T d and d^T d over the pairs, by einsum"""
    pair = idx >= 0
    qd = q[pair].astype(np.float64)
    d, p = qd - after[idx[pair]].astype(np.float64), qd - P.centre(after).astype(np.float64)
    J = jacobians(p)
    H, g, e = np.einsum("kia,kib->kab", J, J), np.einsum("kia,ki->ka", J, d), (d * d).sum(axis=1)
    terms = [H[:, a, b] for a in range(6) for b in range(a, 6)] + [g[:, a] for a in range(6)] + [e]
    return np.array([t.sum() for t in terms]), np.array([np.abs(t).sum() for t in terms])


def test_plane_limit_is_point_to_point_plus_the_plane_terms():
    moving, fixed, normals, Gt = scene("origin")
    kappa = 1.0 / EPS - 1.0
    n64 = normals.astype(np.float64)
    coeff = kappa / (1.0 + kappa * (n64 * n64).sum(axis=1))                      # (I + kappa n n^T)^-1 = I - coeff n n^T
    cov_a = np.stack([(1.0 if a == b else 0.0) - coeff * n64[:, a] * n64[:, b] for a, b in G.TRI], axis=1)
    cov_b = np.zeros((len(moving), 6))
    for R, t in ((None, None), (Gt[:3, :3], Gt[:3, 3])):
        for mode in (K.DIST_CPU_ROUNDING, K.DIST_FMA):
            gs = G.system(moving, cov_b, fixed, cov_a, R, t, mode, LIMIT)
            ps = P.system(moving, fixed, normals, R, t, mode, LIMIT)
            assert np.array_equal(gs["idx"], ps["idx"]) and gs["sums"][29] == ps["sums"][29] > 2000
            pp, pp_abs = point_to_point_terms(gs["q"], fixed, gs["idx"])
            want = pp + kappa * ps["sums"][:28]
            bound = 64 * 2.0 ** -53 * (1.0 / EPS) * (pp_abs + ps["abs"][:28])
            err = np.abs(gs["sums"][:28] - want)
            print("mode %d: worst %.2e of the bound" % (mode, (err / bound).max()))
            assert (err <= bound).all(), (err, bound)
            assert gs["sums"][28] == ps["sums"][28]


def test_identity_covariance_is_the_point_to_point_gauss_newton_step():
    moving, fixed, _, Gt = scene("origin")
    cov_a = np.tile(np.array([1, 0, 0, 1, 0, 1], np.float32), (len(fixed), 1))
    cov_b = np.zeros((len(moving), 6), np.float32)
    start = P.pose44(P.rodrigues([0.0, 0.0, 0.01]), [0.01, 0.0, 0.0]).astype(np.float64)
    R, t = start[:3, :3], start[:3, 3]
    st = G.step(moving, cov_b, fixed, cov_a, R, t, K.DIST_CPU_ROUNDING, LIMIT)
    assert st["stop"] is None
    sy = st["system"]
    pp, _ = point_to_point_terms(sy["q"], fixed, sy["idx"])
    A, g = P.unpack_system(np.concatenate([pp, np.zeros(4)]))
    x = np.linalg.solve(A, -g)
    Rn, tn = P.compose(P.rodrigues(x[:3]), x[3:], sy["centre"], R, t)
    assert np.abs(st["R"] - Rn).max() <= 1e-12 and np.abs(st["t"] - tn).max() <= 1e-12
    assert abs(float(st["error"]) - pp[27] / sy["sums"][29]) <= 1e-7 * pp[27] / sy["sums"][29]


def test_adjugate_inverse_agrees_with_numpy():
    rng = np.random.default_rng(11)
    B = rng.normal(size=(500, 3, 3)) * np.array([1.0, 0.3, 0.05])
    full = np.einsum("kij,klj->kil", B, B) + 1e-4 * np.eye(3)
    S = np.stack([full[:, a, b] for a, b in G.TRI], axis=1)
    M, det = G.inverse_sym3(S)
    want = np.linalg.inv(full)
    cond = np.linalg.cond(full)
    assert (det > 0).all() and 10 < cond.max() < 1e7
    err = np.abs(G.full(M) - want).max(axis=(1, 2)) / np.abs(want).max(axis=(1, 2))
    assert (err <= 1e-12 * cond).all(), (err / cond).max()
    assert np.allclose(det, np.linalg.det(full), rtol=1e-10)
    assert G.inverse_sym3(np.zeros((1, 6)))[1][0] == 0                            # two zero covariances: no pair


def test_plane_covariances_have_the_eigenvalues_eps_one_one():
    rng = np.random.default_rng(2)
    xy = rng.uniform(-1, 1, (300, 2))
    cloud = np.concatenate([xy, (0.2 * xy[:, :1] ** 2 + 0.01 * rng.normal(size=(300, 1)))], axis=1).astype(np.float32)
    for eps in (1e-3, 0.25, 0.0, 1.0):
        out = G.covariances(cloud, 8, G.COV_PLANE, eps)
        assert (out["count"] == 8).all()
        lam = np.linalg.eigvalsh(G.full(out["cov64"]))
        assert np.abs(lam - np.array([np.float64(np.float32(eps)), 1.0, 1.0])).max() <= 1e-12
    raw = G.covariances(cloud, 8, G.COV_RAW)
    _, _, C, count = N.normals(cloud, 8)
    trace = np.trace(C, axis1=1, axis2=2)
    assert np.array_equal(raw["count"], count)
    assert (np.abs(G.full(raw["C"]) - C).max(axis=(1, 2)) <= 16 * 2.0 ** -53 * trace).all()
    # fewer than two neighbours: six zeros in both modes
    for mode in (G.COV_RAW, G.COV_PLANE):
        assert (G.covariances(cloud[:2], 2, mode)["cov"] == 0).all()
