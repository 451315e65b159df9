"""CPU suite: the float64 restatement of the colored ICP (tests/color_reference.py) held to facts that do not depend on it, before the
device is held to the restatement (tests/test_gpu_color.py).

  a linear intensity   on a tilted plane with I = alpha + beta . p the least squares is exact: the gradient is beta's tangential part
  lambda = 1           the linearisation is plane_reference's, sum for sum
  an exact flat plane  texture determines what geometry leaves open: the scaled system is well conditioned at lambda = 0.968 and has a
                       zero diagonal at lambda = 1
  conditioning         how many of the GPU scene's points have a 3 x 3 system too ill conditioned for a per-component bound"""
import numpy as np
import pytest

import color_reference as CR
import knn_reference as K
import plane_reference as P


@pytest.mark.parametrize("k", [8, 16])
def test_a_linear_intensity_on_a_tilted_plane_gives_its_tangential_gradient(k):
    rng = np.random.default_rng(41)
    n = np.array([0.3, -0.2, 0.9])
    n /= np.linalg.norm(n)
    t1 = np.cross(n, [1.0, 0.0, 0.0])
    t1 /= np.linalg.norm(t1)
    t2 = np.cross(n, t1)
    # a spacing of about 1, so that sum u u^T is of the order of the constraint's weight count^2 and cond_1(M) stays below 1e3 (asserted): the
    # solve then loses at most a few 2^-53 cond_1(M) |beta|, two orders inside the bound
    uv = rng.uniform(-12, 12, (600, 2))
    cloud = np.array([0.4, -0.1, 0.7]) + uv[:, :1] * t1 + uv[:, 1:] * t2          # float64: on the plane to rounding
    alpha, beta = 0.3, np.array([0.7, -0.4, 0.25])
    idx, _, count = K.knn(None, cloud.astype(np.float32), k)
    assert (count == k).all()
    e = cloud[idx] - cloud[:, None, :]
    out = CR.solve_neighbourhoods(np.tile(n, (600, 1)), e, e @ beta, count)        # delta = I_j - I_i = beta . e, alpha cancels
    assert alpha == 0.3 and out["solved"].all()
    want = beta - (beta @ n) * n
    err = np.abs(out["d"] - want).max()
    worst = CR.cond1(out["M"]).max()
    print("k %d: worst gradient error %.2e, worst cond_1(M) %.2e" % (k, err, worst))
    assert worst <= 1e3
    assert err <= 1e-12


@pytest.mark.parametrize("name", ["wave", "flat"])
def test_lambda_one_is_the_plane_linearisation(name):
    s = CR.scene(name)
    grad = CR.gradients(s["fixed"], s["normals"], s["ia"], 8)["grad"]
    for R, t in ((None, None), (s["G"][:3, :3], s["G"][:3, 3])):
        got = CR.system(s["moving"], s["ib"], s["fixed"], s["normals"], s["ia"], grad, R, t, K.DIST_CPU_ROUNDING, 0.25, lam=1.0)
        want = P.system(s["moving"], s["fixed"], s["normals"], R, t, K.DIST_CPU_ROUNDING, 0.25)
        assert np.array_equal(got["idx"], want["idx"]) and got["sums"][29] > 2000
        assert (got["sums"] == want["sums"]).all()


def test_texture_determines_an_exact_plane():
    s = CR.scene("flat")
    grad = CR.gradients(s["fixed"], s["normals"], s["ia"], 16)["grad"]
    sy = CR.system(s["moving"], s["ib"], s["fixed"], s["normals"], s["ia"], grad, None, None, K.DIST_CPU_ROUNDING, 0.25, lam=CR.LAMBDA)
    A, _ = P.unpack_system(sy["sums"])
    S, _ = P.scaled(A)
    assert S is not None
    kappa = float(np.linalg.cond(S))
    print("flat, lambda %.3f: cond(S) %.1f from %d pairs" % (CR.LAMBDA, kappa, int(sy["sums"][29])))
    assert kappa <= 1e3
    geometric = CR.system(s["moving"], s["ib"], s["fixed"], s["normals"], s["ia"], grad, None, None, K.DIST_CPU_ROUNDING, 0.25, lam=1.0)
    A1, _ = P.unpack_system(geometric["sums"])
    assert (np.diag(A1)[[2, 3, 4]] == 0).all() and P.scaled(A1)[0] is None        # the rotation about z and the two translations in the plane
    assert CR.step(s["moving"], s["ib"], s["fixed"], s["normals"], s["ia"], grad, np.eye(3), np.zeros(3), K.DIST_CPU_ROUNDING, 0.25, lam=1.0)["stop"] == P.STOP_DEGENERATE


@pytest.mark.parametrize("name", ["wave", "flat"])
def test_few_points_of_the_gradient_scene_are_ill_conditioned(name):
    """the cap tests/test_gpu_color.py leaves out of its per-component bound"""
    g = CR.gradient_scene(name)
    for k in CR.GRADIENT_KS:
        out = CR.gradients(g["cloud"], g["normals"], g["intensity"], k, K.DIST_CPU_ROUNDING, CR.GRADIENT_LIMIT)
        assert (out["grad"][g["zero"]] == 0).all() and (out["grad"][g["line"]] == 0).all() and (out["grad"][g["lonely"]] == 0).all()
        assert out["count"][g["lonely"]] == 0 and (out["count"][g["line"]] == min(k, 3)).all() and not out["solved"][g["line"]].any()
        cond = CR.cond1(out["M"][out["solved"]])
        share = float((cond > CR.ILL_CONDITIONED).mean())
        print("%s k %d: %d solved, cond_1(M) median %.1e max %.1e, share beyond %.0e: %.4f" % (name, k, out["solved"].sum(), np.median(cond), cond.max(),
                                                                                           CR.ILL_CONDITIONED, share))
        assert out["solved"].sum() >= 3900 and share <= CR.ILL_SHARE
