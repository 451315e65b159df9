"""CPU suite: tests/ndt_reference.py, the float64 restatement the GPU suite of mi_ndt_* is held against, held to its own invariants --
the constants' closed form, C' M = I, the eigenvalue floor, a weight that falls with m -- and to whole registrations on the scenes of
tests/test_gpu_plane.py: it has to converge there before anything is compared with it.  The residual it ends with (a few 1e-4 in the
rotation, about 1e-3 in the translation) is NDT's own model bias on a curved surface, not an error."""
import functools
import math

import numpy as np
import pytest

import gicp_reference as G
import ndt_reference as N
from test_gpu_plane import EPS_TRANSLATION, distance, scene


@functools.lru_cache(maxsize=None)
def scene_map(name, voxel):
    return N.voxels(scene(name)[1], voxel)


@functools.lru_cache(maxsize=None)
def reference_run(name, voxel, neighbourhood):
    return N.register(scene(name)[0], scene_map(name, voxel), 1e-6, EPS_TRANSLATION[name], 50, neighbourhood)


def test_the_constants_closed_form():
    c1, c2 = 10 * (1 - float(np.float32(0.55))), float(np.float32(0.55))
    d3 = -math.log(c2)
    d1 = -math.log(c1 + c2) - d3
    d2 = -2 * math.log((-math.log(c1 * math.exp(-0.5) + c2) - d3) / d1)
    got = N.constants(1.0, 0.55)
    assert np.allclose(got, [d1, d2, -d2 / 2, -d1 * d2], rtol=1e-14, atol=0)
    assert got[0] < 0 < got[1] and got[3] > 0
    # the score of a point at its voxel's mean is -d1, and one Mahalanobis unit away it has fallen to the mixture's value there
    assert np.isclose(-got[0] * np.exp(got[2] * 1.0), math.log(c1 * math.exp(-0.5) + c2) + d3)


@pytest.mark.parametrize("voxel", [0.5, 1.0])
def test_voxel_distributions(voxel):
    vox = scene_map("origin", voxel)
    has = vox["has"]
    assert np.array_equal(has, N.has_distribution(vox)) and has.sum() > 10
    assert (vox["count"].sum(), (np.diff(np.lexsort(vox["coord"].T[[0, 1, 2]])) == 1).all()) == (4000, True)      # rows ascend by (cz, cy, cx)
    M, Cp = G.full(vox["M64"][has]), G.full(vox["cov64"][has])
    assert np.abs(M @ Cp - np.eye(3)).max() <= 1e-10
    lam = np.linalg.eigvalsh(Cp)
    assert (lam[:, 0] >= float(np.float32(0.01)) * lam[:, 2] * (1 - 1e-12)).all() and vox["raised"][has].any()
    assert (vox["icov"][~has] == 0).all() and (vox["cov"][~has] == 0).all() and (vox["count"][~has] < 6).all()
    loose = N.voxels(scene("origin")[1], voxel, eig_ratio=1e-30)
    assert not loose["raised"][loose["has"]].any() and np.array_equal(loose["cov64"][loose["has"]], loose["C"][loose["has"]])


def test_prototype_voxel_counts():
    vox = scene_map("origin", 0.5)
    assert (len(vox["count"]), int((vox["count"] < 6).sum())) == (78, 7)


def test_a_terms_weight_falls_with_m():
    h, k = N.constants(0.5)[2:]
    M = np.tile(np.array([[2.0, 0.1, 0, 3.0, 0, 1.5]]), (50, 1))
    q = np.linspace(0, 2, 50)[:, None] * np.array([[1.0, 0.5, -0.25]])
    t = N.term(q, np.zeros((50, 3)), M, h, k)
    assert t["ok"].all() and (np.diff(t["m"]) > 0).all() and (np.diff(t["w"]) < 0).all() and t["e"][0] == 1 and (t["w"] > 0).all()
    assert not N.term(q[1:2], np.zeros((1, 3)), -M[:1], h, k)["ok"][0] and not N.term(q[1:2], np.zeros((1, 3)), 0 * M[:1], h, k)["ok"][0]


@pytest.mark.parametrize("name,voxel,neighbourhood", [("origin", 0.5, 1), ("origin", 0.5, 7), ("origin", 1.0, 7), ("shifted", 0.5, 7), ("shifted", 0.5, 1)])
def test_whole_runs_converge(name, voxel, neighbourhood):
    run = reference_run(name, voxel, neighbourhood)
    Gt = scene(name)[3]
    dR, dt = distance(run["R"], run["t"], Gt)
    kappa = max(s["kappa"] for s in run["steps"])
    print("%s voxel %g neighbourhood %d: %d voxels, %d terms at the start, %d at the end, %d iterations, |dR| %.2e |dt| %.2e, score %.4f, cond(S) <= %.2f" % (
        name, voxel, neighbourhood, len(scene_map(name, voxel)["count"]), run["steps"][0]["system"]["sums"][29], run["steps"][-1]["system"]["sums"][29],
        run["iterations"], dR, dt, run["score"], kappa))
    assert run["stop"] == N.STOP_CONVERGED and run["iterations"] <= 25
    assert 0 < run["score"] <= 1 and kappa <= 100
