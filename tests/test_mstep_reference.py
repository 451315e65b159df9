"""CPU suite: the float64 M-step reference of tests/mstep_reference.py against the reference's own M-step on the bunny fixture, and its
parts against what they must be by construction."""
import numpy as np
import pytest

import mstep_reference as M


@pytest.mark.parametrize("const_scale,key", [(False, "mstep0_scale_free"), (True, "mstep0_const_scale")])
def test_moments_and_solve_match_the_fixture(golden, bunny, const_scale, key):
    # the fixture's own bars (tests/test_gpu_cpd.py test_mstep_matches_golden)
    before, after = bunny
    g = golden.json("bunny_cpd.json")[key]
    e = golden.npz("bunny_cpd_estep0.npz")
    xs, ks, xs_abs, ks_abs = M.moments(before, after, e["p1"], e["pt1"], e["px"])
    assert np.isnan(xs[0]) and np.isfinite(xs[1:]).all() and np.isfinite(ks).all()
    assert (np.abs(xs[1:]) <= xs_abs[1:]).all() and (np.abs(ks) <= ks_abs).all()
    s = M.solve(xs, ks, const_scale, 1.0)
    assert np.abs(s["R"] - np.array(g["R"])).max() < 1e-5
    assert np.abs(s["t"] - np.array(g["t"])).max() < 1e-4
    assert abs(s["scale"] - g["scale"]) < 1e-4 * g["scale"]
    assert abs(s["sigma2"] - g["sigma2"]) < 1e-3 * g["sigma2"] + 5e-5
    assert abs(np.linalg.det(s["R"]) - 1.0) < 1e-12 and np.abs(s["R"] @ s["R"].T - np.eye(3)).max() < 1e-12


def test_moments_are_the_plain_sums():
    rng = np.random.default_rng(5)
    m, n = 37, 23
    b, a = rng.normal(size=(m, 3)).astype(np.float32), rng.normal(size=(n, 3)).astype(np.float32)
    p1, pt1, px = rng.uniform(0, 1, m).astype(np.float32), rng.uniform(0, 1, n).astype(np.float32), rng.normal(size=(m, 3)).astype(np.float32)
    xs, ks, xs_abs, ks_abs = M.moments(b, a, p1, pt1, px)
    bd, ad = b.astype(np.float64), a.astype(np.float64)
    assert np.allclose(xs[1:4], ad.T @ pt1, rtol=1e-14) and np.isclose(xs[4], ((ad ** 2).sum(1) * pt1).sum(), rtol=1e-14)
    assert np.isclose(ks[0], p1.astype(np.float64).sum(), rtol=1e-14) and np.allclose(ks[1:4], bd.T @ p1, rtol=1e-13, atol=1e-14)
    assert np.allclose(ks[4:13].reshape(3, 3), bd.T @ px.astype(np.float64), rtol=1e-13, atol=1e-14)
    assert np.isclose(ks[13], ((bd ** 2).sum(1) * p1).sum(), rtol=1e-14)
    # rows with P1 = 0 and PX = 0 contribute exactly nothing
    p1[::2], px[::2] = 0, 0
    full = M.moments(b, a, p1, pt1, px)
    part = M.moments(b[1::2], a, p1[1::2], pt1, px[1::2])
    assert np.array_equal(full[1], part[1]) and np.array_equal(full[3], part[3])


def test_solve_recovers_a_similarity():
    # hard assignments (P = a permutation): the M-step is the Procrustes solution, exact for a = s R b + t
    rng = np.random.default_rng(9)
    b = rng.uniform(-5, 5, (200, 3)).astype(np.float32)
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    q *= np.sign(np.linalg.det(q))
    a = (1.7 * b.astype(np.float64) @ q.T + [0.5, -1.0, 2.0]).astype(np.float32)
    xs, ks, _, _ = M.moments(b, a, np.ones(200, np.float32), np.ones(200, np.float32), a)
    s = M.solve(xs, ks, False)
    assert np.abs(s["R"] - q).max() < 1e-6 and abs(s["scale"] - 1.7) < 1e-6 and np.abs(s["t"] - [0.5, -1.0, 2.0]).max() < 1e-5
    assert s["sigma2"] < 1e-9
    assert s["sigmaSubtrahend"] > 0 and s["scaleDenominator"] > 0 and s["scaleNumerator"] > 0
    # a reflection: the determinant rule keeps R a rotation
    xs, ks, _, _ = M.moments(b, a * np.float32([1, 1, -1]), np.ones(200, np.float32), np.ones(200, np.float32), a * np.float32([1, 1, -1]))
    assert abs(np.linalg.det(M.solve(xs, ks, False)["R"]) - 1.0) < 1e-12


def test_sigma2_exact_is_the_bunny_value_and_has_no_cancellation(bunny):
    before, after = bunny
    s2 = M.sigma2_exact(before, after)
    assert abs(s2 - 12.943) < 1e-2                                  # tests/test_gpu_cpd.py test_sigma_squared_is_the_exact_value
    rng = np.random.default_rng(3)
    b, a = rng.uniform(0, 1, (40, 3)).astype(np.float32), rng.uniform(0, 1, (55, 3)).astype(np.float32)
    brute = ((a.astype(np.float64)[:, None, :] - b.astype(np.float64)[None, :, :]) ** 2).sum() / (3.0 * 40 * 55)
    assert abs(M.sigma2_exact(b, a) - brute) < 1e-14 * brute
    off = np.float32([100, -50, 30])
    bo, ao = b + off, a + off
    brute = ((ao.astype(np.float64)[:, None, :] - bo.astype(np.float64)[None, :, :]) ** 2).sum() / (3.0 * 40 * 55)
    assert abs(M.sigma2_exact(bo, ao) - brute) < 1e-13 * brute
    assert M.U32 < M.sigma2_init_bound(b - np.float32(0.5), a - np.float32(0.5)) < M.sigma2_init_bound(bo, ao) < 2 * M.U32


def test_transform_is_float32_in_the_kernels_order():
    rng = np.random.default_rng(4)
    b = rng.uniform(-5, 5, (10, 3)).astype(np.float32)
    R, t, s = rng.normal(size=(3, 3)).astype(np.float32), rng.normal(size=3).astype(np.float32), np.float32(1.3)
    y = M.transform(b, R, t, s)
    assert y.dtype == np.float32
    i = 7
    x0 = np.float32(np.float32(R[1, 0] * b[i, 0]) + np.float32(R[1, 1] * b[i, 1]))
    assert y[i, 1] == np.float32(np.float32(s * np.float32(x0 + np.float32(R[1, 2] * b[i, 2]))) + t[1])
    assert np.abs(y - (s * b.astype(np.float64) @ R.astype(np.float64).T + t)).max() < 1e-5


def test_row_and_chain_counts_follow_the_constants():
    assert [M.sum_rows(p, "post") for p in (1, 64, 65, 32768, 32769)] == [1, 1, 2, 512, 512]
    assert [M.sum_rows(p, "standalone") for p in (1, 256, 257, 131072, 131073)] == [1, 1, 2, 512, 512]
    assert [M.sum_rows(p, "trunc") for p in (1, 64, 65, 262144, 262145)] == [1, 1, 2, 4096, 4096]
    # one trip below the cap, a second one for the wrapped row just past it
    assert M.additions(32768, "post", 16) + 1 == M.additions(32769, "post", 16)
    assert M.additions(262144, "trunc", 8) + 1 == M.additions(262145, "trunc", 8)
    assert M.additions(131072, "standalone", 8) + 1 == M.additions(131073, "standalone", 8)
    assert M.additions(1, "post", 8) == 1 + 9 + 1 + 32 and M.additions(1, "trunc", 16) == 1 + 6 + 1 + 16
