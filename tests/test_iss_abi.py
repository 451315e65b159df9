"""CPU suite: the ISS keypoint entry points exist, the argument errors that need no device are refused, the defaults are the documented
ones, and the restatement the GPU tests use as their oracle (tests/iss_reference.py) gives the answers worked by hand on the 3 x 3 x 3
integer lattice of tests/test_knn_abi.py, an exact plane, identical points, a single point and a tied pair."""
import ctypes as C

import numpy as np
import pytest

import iss_reference as I
import knn_reference as K
from test_knn_abi import lattice3

MODES = [K.DIST_CPU_ROUNDING, K.DIST_FMA]


def test_library_exports_the_iss_entry_points(capi):
    lib = capi.lib()
    for name in ("mi_iss_keypoints", "mi_iss_keypoints_times", "mi_iss_params_default"):
        assert hasattr(lib, name), name
        assert name in capi.EXPORTS, name
    assert lib.mi_abi_version() == 4          # additive: no signature of version 4 changed
    assert C.sizeof(capi.IssParams) == 64


def test_a_null_context_is_refused_without_a_device(capi):
    cloud = np.zeros((4, 3), np.float32)
    xyz, index, flag = np.full((4, 3), -7.5, np.float32), np.full(4, -7, np.int32), np.full(4, 7, np.uint8)
    saliency, eigenvalues, neighbours = np.full(4, -7.5, np.float32), np.full((4, 3), -7.5, np.float32), np.full(4, -7, np.int32)
    out_n = C.c_int(-7)
    p = capi.iss_params(salient_radius=1.0, non_max_radius=1.0)
    rc = capi.iss_keypoints_raw(None, cloud.ctypes.data, 4, C.addressof(p), xyz.ctypes.data, index.ctypes.data, C.addressof(out_n), flag.ctypes.data,
                                saliency.ctypes.data, eigenvalues.ctypes.data, neighbours.ctypes.data)
    msg = capi.lib().mi_last_error().decode()
    assert rc == capi.MI_ERR_INVALID_ARG and msg.startswith("mi_iss_keypoints") and "null context" in msg
    assert (xyz == -7.5).all() and (index == -7).all() and (flag == 7).all() and (saliency == -7.5).all() and (eigenvalues == -7.5).all()
    assert (neighbours == -7).all() and out_n.value == -7
    out = (C.c_double * 8)()
    f = capi.lib().mi_iss_keypoints_times
    f.argtypes, f.restype = [C.c_void_p, C.c_void_p], C.c_int
    assert f(None, out) == capi.MI_ERR_INVALID_ARG


def test_defaults_are_the_documented_ones(capi):
    p = capi.iss_params()
    assert (p.salient_radius, p.non_max_radius) == (0.0, 0.0)                  # the caller must set both
    assert (p.gamma_21, p.gamma_32) == (float(np.float32(0.975)), float(np.float32(0.975)))
    assert (p.min_neighbours, p.dist_mode) == (5, capi.DIST_CPU_ROUNDING) and list(p.reserved) == [0] * 10
    q = capi.iss_params(salient_radius=0.9, non_max_radius=0.6, min_neighbours=3, dist_mode=capi.DIST_FMA)
    assert (q.salient_radius, q.non_max_radius) == (float(np.float32(0.9)), float(np.float32(0.6)))
    assert (q.min_neighbours, q.dist_mode, q.gamma_21) == (3, capi.DIST_FMA, float(np.float32(0.975)))
    with pytest.raises(AttributeError):
        capi.iss_params(no_such_field=1)


@pytest.mark.parametrize("mode", MODES)
def test_restatement_on_a_lattice_worked_by_hand(mode):
    L = lattice3()                                                    # index = x + 3 y + 9 z
    on_boundary = ((L == 0) | (L == 2)).sum(axis=1)                   # 3: corner, 2: edge, 1: face, 0: the centre
    # radius 1: the face neighbours inside the lattice -- 3 at a corner, 4 on an edge, 5 on a face, 6 at the centre; all of them AT the radius
    ref = I.saliency(L, 1.0, mode, min_neighbours=3)
    assert ref["count"].tolist() == (6 - on_boundary).tolist() and sorted(set(ref["count"].tolist())) == [3, 4, 5, 6]
    assert (I.saliency(L, np.nextafter(np.float32(1), np.float32(0)), mode)["count"] == 0).all()
    # the centre: d = +-e_a, S = 0, Q = 2 I, c = 7: C = 2/7 I, three equal eigenvalues, so lambda1 < gamma lambda2 fails
    assert np.abs(ref["lam"][13] - 2.0 / 7).max() <= 1e-15 and not ref["gate"][13]
    # a corner: d = e_x, e_y, e_z, S = (1, 1, 1), Q = I, c = 4: C = I / 4 - 1 1^T / 16, eigenvalues 1/16 (along 1) and 1/4 twice: fails too
    assert np.abs(ref["lam"][0] - [1.0 / 16, 0.25, 0.25]).max() <= 1e-15 and not ref["gate"][0]
    # the edge point (1, 0, 0): d = +-e_x, e_y, e_z, S = (0, 1, 1), Q = diag(2, 1, 1), c = 5: C = diag(2/5, 1/5, 1/5) - (0, 1, 1)(0, 1, 1)^T / 25,
    # eigenvalues 1/5 - 2/25 = 3/25 (along (0, 1, 1)), 1/5 and 2/5: both ratio tests hold, so it is a candidate with saliency 3/25
    assert np.abs(ref["lam"][1] - [3.0 / 25, 0.2, 0.4]).max() <= 1e-15 and ref["gate"][1]
    assert ref["saliency"][1] == np.float32(ref["lam"][1, 0]) and abs(float(ref["saliency"][1]) - 0.12) <= 6e-8 * 0.12
    # ... but not with min_neighbours above its four
    assert not I.saliency(L, 1.0, mode, min_neighbours=5)["gate"][1]
    # the face centre (1, 1, 0): d = +-e_x, +-e_y, e_z, S = (0, 0, 1), Q = diag(2, 2, 1), c = 6: C = diag(1/3, 1/3, 1/6 - 1/36): lambda1 = lambda2
    assert np.abs(ref["lam"][4] - [5.0 / 36, 1.0 / 3, 1.0 / 3]).max() <= 1e-15 and not ref["gate"][4]
    # so the candidates are the twelve edge points, all with one saliency to rounding; no two of them are within radius 1 of each
    # other, but at radius sqrt 2 each has edge neighbours (e.g. (1, 0, 0) and (0, 1, 0))
    assert np.flatnonzero(ref["saliency"] > 0).tolist() == np.flatnonzero(on_boundary == 2).tolist()


@pytest.mark.parametrize("mode", MODES)
def test_restatement_on_degenerate_clouds(mode):
    rng = np.random.default_rng(5)
    plane = rng.uniform(-5, 5, (400, 3)).astype(np.float32)
    plane[:, 2] = 0.75                                                # an exact plane: lambda0 = 0 exactly, no candidate
    ref, key = I.keypoints(plane, 1.5, 1.0, mode)
    assert ref["count"].mean() > 15 and (ref["lam"][:, 0] == 0).all() and not (ref["saliency"] > 0).any() and not key.any()
    same = np.tile(np.array([[1.5, -2.25, 3.0]], np.float32), (200, 1))   # identical points: every other one is a neighbour, C = 0
    ref, key = I.keypoints(same, 1.0, 1.0, mode)
    assert (ref["count"] == 199).all() and (ref["lam"] == 0).all() and not ref["gate"].any() and not key.any()
    ref, key = I.keypoints(same[:1], 1.0, 1.0, mode, min_neighbours=1)    # a single point
    assert ref["count"].tolist() == [0] and ref["lam"].tolist() == [[0.0, 0.0, 0.0]] and ref["saliency"].tolist() == [0.0] and key.tolist() == [False]


@pytest.mark.parametrize("mode", MODES)
def test_restatement_of_the_suppression_on_a_tied_pair(mode):
    # five points on a line, one apart; non-max radius 1: the ball of point i is {i - 1, i + 1}
    line = np.stack([np.arange(5, dtype=np.float32), np.zeros(5, np.float32), np.zeros(5, np.float32)], axis=1)
    s = np.array([0.1, 0.5, 0.5, 0.2, 0.3], np.float32)
    # 1 and 2 are tied and in each other's ball: the lower index survives (a strict ">" would drop both); 4 beats its one neighbour
    assert I.nms(s, line, 1.0, 1, mode).tolist() == [False, True, False, False, True]
    assert I.nms(s, line, 1.0, 2, mode).tolist() == [False, True, False, False, False]      # (4 has one neighbour only)
    assert I.nms(s, line, 1.0, 1, mode, only=[2, 4]).tolist() == [False, True]
    # the same values out of each other's reach: both survive
    assert I.nms(np.array([0.5, 0.1, 0.5, 0.1, 0.1], np.float32), line, 1.0, 1, mode).tolist() == [True, False, True, False, False]
    # a zero is never a keypoint, whatever surrounds it
    assert I.nms(np.zeros(5, np.float32), line, 1.0, 1, mode).tolist() == [False] * 5
    # a point AT the radius belongs: at the float below 1 nobody has a neighbour, and min_neighbours = 1 leaves nothing
    assert not I.nms(s, line, np.nextafter(np.float32(1), np.float32(0)), 1, mode).any()
