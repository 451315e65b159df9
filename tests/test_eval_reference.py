"""CPU suite: the restatement the GPU tests of mi_evaluate_registration use as their oracle (tests/eval_reference.py) gives the answers
worked by hand on a 3 x 3 lattice: points (x, y, 0), x and y in {0, 1, 2}, index x + 3 y."""
import numpy as np
import pytest

import eval_reference as E
import knn_reference as K
import plane_reference as P

MODES = [K.DIST_CPU_ROUNDING, K.DIST_FMA]


def lattice():
    g = np.arange(3, dtype=np.float32)
    y, x = np.meshgrid(g, g, indexing="ij")
    return np.stack([x.ravel(), y.ravel(), np.zeros(9, np.float32)], axis=1)


@pytest.mark.parametrize("mode", MODES)
def test_the_lattice_against_itself(mode):
    fixed = lattice()
    ev = E.evaluate(fixed, fixed, dist_mode=mode)
    assert ev["idx"].tolist() == list(range(9)) and (ev["d2"] == 0).all()
    assert ev["fitness"] == 1.0 and ev["rmse"] == 0.0
    s = ev["sums"]
    assert s[29] == 9 and s[27] == 0 and s[28] == 0 and (s[30:] == 0).all()
    L, g = P.unpack_system(s)
    assert np.array_equal(L, ev["information"]) and np.array_equal(L, L.T)
    assert np.array_equal(L[3:, 3:], 9 * np.eye(3))
    # sum x^2 = sum y^2 = 15, sum x y = 9, z = 0: sum (|a|^2 I - a a^T) by hand, and by numpy
    a = fixed.astype(np.float64)
    assert np.array_equal(L[:3, :3], np.array([[15.0, -9.0, 0.0], [-9.0, 15.0, 0.0], [0.0, 0.0, 30.0]]))
    assert np.array_equal(L[:3, :3], (a * a).sum() * np.eye(3) - a.T @ a)
    # the mixed block: sum [a]x, with sum a = (9, 9, 0)
    assert np.array_equal(L[:3, 3:], np.array([[0.0, 0.0, 9.0], [0.0, 0.0, -9.0], [-9.0, 9.0, 0.0]]))
    assert np.array_equal(g, np.zeros(6))


@pytest.mark.parametrize("mode", MODES)
def test_the_lattice_shifted_along_x(mode):
    fixed = lattice()
    moving = fixed + np.array([0.25, 0, 0], np.float32)
    for ev in (E.evaluate(moving, fixed, dist_mode=mode), E.evaluate(fixed, fixed, np.eye(3), [0.25, 0, 0], dist_mode=mode)):
        # every moving point is 0.25 from its own lattice point and 0.75 from the next
        assert ev["idx"].tolist() == list(range(9)) and (ev["d2"] == np.float32(0.0625)).all()
        assert ev["fitness"] == 1.0 and ev["rmse"] == 0.25
        s = ev["sums"]
        assert s[27] == 9 * 0.0625 and s[28] == 9 * 0.0625 and s[29] == 9
        # g = sum G^T d: the translation part is sum d, the rotation part sum a x d = (0, 0, -0.25 sum a_y)
        assert s[21:27].tolist() == [0.0, 0.0, -2.25, 2.25, 0.0, 0.0]
        # one Gauss-Newton step takes the shift back: x = (0, 0, 0, -0.25, 0, 0) solves Lambda x = -g
        x = np.linalg.solve(ev["information"], -s[21:27])
        assert np.abs(x - np.array([0, 0, 0, -0.25, 0, 0])).max() <= 1e-14
    # a limit below the shift drops every pair
    ev = E.evaluate(moving, fixed, dist_mode=mode, max_d2=0.01)
    assert (ev["idx"] == -1).all() and np.isposinf(ev["d2"]).all()
    assert ev["fitness"] == 0.0 and ev["rmse"] == 0.0 and (ev["sums"] == 0).all() and (ev["information"] == 0).all()
    # ... and a limit AT the distance keeps them
    assert E.evaluate(moving, fixed, dist_mode=mode, max_d2=0.0625)["fitness"] == 1.0


@pytest.mark.parametrize("mode", MODES)
def test_ties_and_given_pairs(mode):
    fixed = lattice()
    # half way between points 0 and 1, and between 4 and 7: the lower index
    ev = E.evaluate(np.array([[0.5, 0, 0], [1, 1.5, 0]], np.float32), fixed, dist_mode=mode)
    assert ev["idx"].tolist() == [0, 4] and (ev["d2"] == np.float32(0.25)).all()
    # given pairs: -1 is no pair, a pair beyond the limit is dropped, the others are taken as they come (not the nearest)
    moving = fixed + np.array([0.25, 0, 0], np.float32)
    pairs = np.array([1, -1, 2, 3, 4, 5, 8, 7, 8], np.int32)
    ev = E.evaluate(moving, fixed, pairs=pairs, dist_mode=mode, max_d2=1.0)
    assert ev["idx"].tolist() == [1, -1, 2, 3, 4, 5, -1, 7, 8]                 # 6 -> 8 is (1.75, 0): 3.0625 away
    assert ev["d2"].tolist() == [0.5625, np.inf, 0.0625, 0.0625, 0.0625, 0.0625, np.inf, 0.0625, 0.0625]
    assert ev["fitness"] == 7 / 9 and ev["sums"][28] == 0.5625 + 6 * 0.0625 and ev["sums"][27] == ev["sums"][28]
    # given the search's own answer, the restatement repeats itself
    a, b = E.evaluate(moving, fixed, dist_mode=mode, max_d2=1.0), None
    b = E.evaluate(moving, fixed, pairs=a["idx"], dist_mode=mode, max_d2=1.0)
    assert np.array_equal(a["sums"], b["sums"]) and np.array_equal(a["idx"], b["idx"]) and np.array_equal(a["d2"].view(np.uint32), b["d2"].view(np.uint32))
