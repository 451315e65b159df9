"""CPU suite: the restatement the GPU tests of mi_mls_smooth use as their oracle (tests/mls_reference.py), held to facts that do not depend
on it: answers worked by hand on an exact lattice plane and on the smallest balls, the freedom the rules leave (the frame turned about the
normal moves the outputs by rounding alone), and the reason the call exists -- on a noisy surface the order-2 output is closer to the
noise-free surface than the input is."""
import numpy as np
import pytest

import knn_reference as K
import mls_reference as M
from test_gpu_iss import surface_recipe

MODES = [K.DIST_CPU_ROUNDING, K.DIST_FMA]
U = 2.0 ** -53


def lattice_plane(side, z):
    g = np.arange(side, dtype=np.float32)
    y, x = np.meshgrid(g, g, indexing="ij")
    return np.stack([x.ravel(), y.ravel(), np.full(side * side, z, np.float32)], axis=1)      # index = x + side y


@pytest.mark.parametrize("mode", MODES)
def test_restatement_on_a_lattice_plane_worked_by_hand(mode):
    P = lattice_plane(5, 0.75)
    on_boundary = ((P[:, :2] == 0) | (P[:, :2] == 4)).sum(axis=1)
    # radius 1: the point and its face neighbours inside the lattice -- 3 at a corner, 4 on an edge, 5 inside; all neighbours AT the radius
    ref = M.smooth(P, 1.0, mode)
    assert ref["neighbours"].tolist() == (5 - on_boundary).tolist()
    assert (M.smooth(P, np.nextafter(np.float32(1), np.float32(0)), mode)["neighbours"] == 1).all()
    # fewer than six points: the plane everywhere; every d_z is 0, so lambda0 = 0, the normal is +-e_z and the foot is the query
    assert (ref["status"] == M.PLANE).all() and (ref["lam"][:, 0] == 0).all() and (ref["curvature"] == 0).all()
    assert np.array_equal(ref["xyz"].view(np.uint32), P.view(np.uint32)) and (np.abs(ref["normals"][:, 2]) == 1).all() and (ref["normals"][:, :2] == 0).all()
    # an interior point: d = 0, +-e_x, +-e_y: S = 0, Q = diag(2, 2, 0), c = 5: eigenvalues 0, 2/5, 2/5
    assert np.abs(ref["lam"][12] - [0.0, 0.4, 0.4]).max() <= 1e-15
    # radius sqrt 2 (the next float up: the points at d2 = 2 belong): nine points inside, six on an edge, four at a corner
    r = float(np.nextafter(np.sqrt(np.float32(2)), np.float32(2)))
    ref = M.smooth(P, r, mode)
    assert sorted(set(ref["neighbours"].tolist())) == [4, 6, 9] and ref["neighbours"][12] == 9
    # four points: the plane; nine: the quadratic of heights that are all 0, which is 0; six on an edge: a = 0, 1 (or -1, 0) only along one
    # axis, so a a = +-a there and the system is degenerate -- the plane again.  The input's bits in every case.
    assert set(ref["status"][ref["neighbours"] == 4].tolist()) == {M.PLANE} and set(ref["status"][ref["neighbours"] == 9].tolist()) == {M.QUADRATIC}
    assert set(ref["status"][ref["neighbours"] == 6].tolist()) == {M.PLANE} and (ref["pivot"][ref["neighbours"] == 6] < M.PIVOT_MIN).all()
    assert np.array_equal(ref["xyz"].view(np.uint32), P.view(np.uint32)) and (np.abs(ref["normals"][:, 2]) == 1).all()
    # min_neighbours above the ball: untouched, a zero normal
    ref = M.smooth(P, 1.0, mode, min_neighbours=5)
    assert (ref["status"] == np.where(on_boundary == 0, M.PLANE, M.UNTOUCHED)).all()
    assert (ref["normals"][on_boundary > 0] == 0).all() and np.array_equal(ref["xyz"].view(np.uint32), P.view(np.uint32))
    # a separate query above the plane comes down onto it, and its own copy is NOT in the ball
    q = np.array([[2.0, 2.0, 1.0]], np.float32)
    ref = M.smooth(P, 1.25, mode, queries=q)
    assert ref["neighbours"].tolist() == [5] and ref["status"].tolist() == [M.PLANE] and ref["xyz"].tolist() == [[2.0, 2.0, 0.75]]


@pytest.mark.parametrize("mode", MODES)
def test_restatement_on_degenerate_clouds(mode):
    same = np.tile(np.array([[1.5, -2.25, 3.0]], np.float32), (200, 1))
    ref = M.smooth(same, 1.0, mode)
    assert (ref["neighbours"] == 200).all() and (ref["status"] == M.PLANE).all() and (ref["lam"] == 0).all() and (ref["pivot"] == 0).all()
    assert np.array_equal(ref["xyz"].view(np.uint32), same.view(np.uint32)) and (ref["curvature"] == 0).all()
    line = np.stack([np.arange(9), 2.0 * np.arange(9), np.zeros(9)], axis=1).astype(np.float32)
    ref = M.smooth(line, 40.0, mode)
    assert (ref["status"] == M.PLANE).all() and np.isfinite(ref["xyz"]).all() and np.isfinite(ref["normals"]).all()
    assert np.abs(ref["xyz64"] - line).max() <= 1e-13                         # a point of the line is its own foot
    ref = M.smooth(line[:2], 40.0, mode)
    assert (ref["status"] == M.UNTOUCHED).all() and (ref["neighbours"] == 2).all() and (ref["normals"] == 0).all()


def test_turning_the_frame_about_the_normal_moves_the_outputs_by_rounding_alone():
    """Bound: 4 (c + 8) 2^-53 radius / pivot -- every one of the c terms of the 27 sums is rounded differently in the turned basis, the
    shape of a change of summation order; measured 0.16 of the bound's unit at its worst."""
    cloud = surface_recipe(np.random.default_rng(131), 2400, 0, 5)
    ref = M.smooth(cloud, 0.9, K.DIST_CPU_ROUNDING)
    assert (ref["status"] == M.QUADRATIC).all() and ref["pivot"].min() > 1e-6
    unit = (ref["neighbours"] + 8) * U * float(np.float32(0.9)) / ref["pivot"]
    for angle in (0.7, 2.0, -3.0):
        rot = M.smooth(cloud, 0.9, K.DIST_CPU_ROUNDING, frame_rotation=angle)
        assert np.array_equal(rot["status"], ref["status"]) and np.array_equal(rot["neighbours"], ref["neighbours"])
        ex, en = np.abs(rot["xyz64"] - ref["xyz64"]).max(axis=1) / unit, np.abs(rot["normals64"] - ref["normals64"]).max(axis=1) / unit
        print("frame turned by %g: xyz moves %.3f, normals %.3f of (c + 8) 2^-53 radius / pivot at the worst" % (angle, ex.max(), en.max()))
        assert ex.max() <= 4 and en.max() <= 4
        assert np.array_equal(rot["curvature"], ref["curvature"])             # (the plane does not know the frame)


def surface_distance(p):
    """signed distance of points to z = 0.6 sin(1.3 x) cos(1.1 y), to first order: the height's residual over the gradient's length"""
    p = np.asarray(p, np.float64)
    x, y = p[:, 0], p[:, 1]
    f = 0.6 * np.sin(1.3 * x) * np.cos(1.1 * y)
    fx, fy = 0.78 * np.cos(1.3 * x) * np.cos(1.1 * y), -0.66 * np.sin(1.3 * x) * np.sin(1.1 * y)
    return (p[:, 2] - f) / np.sqrt(1 + fx * fx + fy * fy)


def test_the_quadratic_brings_a_noisy_surface_closer_to_the_noise_free_one():
    cloud = surface_recipe(np.random.default_rng(131), 2400, 0, 5)               # sigma = 0.01 on the heights
    before = np.sqrt((surface_distance(cloud) ** 2).mean())
    for radius in (0.5, 0.7, 0.9):
        ref = M.smooth(cloud, radius, K.DIST_CPU_ROUNDING)
        assert (ref["status"] != M.UNTOUCHED).all() and (ref["status"] == M.QUADRATIC).mean() > 0.99
        after = np.sqrt((surface_distance(ref["xyz"]) ** 2).mean())
        flat = np.sqrt((surface_distance(M.smooth(cloud, radius, K.DIST_CPU_ROUNDING, order=1)["xyz"]) ** 2).mean())
        print("radius %g: RMS distance to the noise-free surface %.5f before, %.5f after order 2 (ratio %.3f), %.5f after order 1 (ratio %.3f)" % (
            radius, before, after, after / before, flat, flat / before))
        assert after < before
        assert after < flat                                                   # (the surface is curved: the plane alone flattens it)
    assert 0.008 < before < 0.01
