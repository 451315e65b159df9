"""CPU suite: the plane-segmentation entry points exist, a NULL context is refused without a device with every output untouched, and the
restatement the GPU tests use as their oracle (tests/segment_reference.py) gives the answers worked by hand on the 3 x 3 x 3 integer lattice
of tests/test_knn_abi.py, collinear and identical points, an integer plane, three planted planes handed over interleaved, and a small
horizontal plane in front of a larger vertical one under the axis rule."""
import ctypes as C

import numpy as np

import segment_reference as R
from test_knn_abi import lattice3


def test_library_exports_the_segment_entry_points(capi):
    lib = capi.lib()
    for name in ("mi_segment_plane", "mi_segment_plane_hypotheses", "mi_segment_plane_times"):
        assert hasattr(lib, name), name
        assert name in capi.EXPORTS, name
    assert lib.mi_abi_version() == 4          # additive: no signature of version 4 changed
    text = open(capi._HEADER).read()
    assert "#define MI_SEGMENT_MAX_PLANES 16" in text and "#define MI_SEGMENT_STAGES 8" in text
    assert capi.SEGMENT_MAX_PLANES == 16
    for name in ("segment_plane", "segment_plane_hypotheses", "segment_plane_times"):
        assert callable(getattr(capi.Context, name))
    assert callable(capi.segment_plane_raw) and callable(capi.segment_plane_hypotheses_raw)


def test_a_null_context_is_refused_without_a_device(capi):
    cloud = np.zeros((4, 3), np.float32)
    planes, inl, labels = np.full(8, -7, np.float32), np.full(2, -7, np.int32), np.full(4, -7, np.int32)
    rmse, winners, found = np.full(2, -7, np.float32), np.full(2, -7, np.int32), C.c_int(-7)
    rc = capi.segment_plane_raw(None, cloud.ctypes.data, 4, 0.1, 10, 0, 2, 2, 3, None, 0.0, planes.ctypes.data, C.addressof(found), inl.ctypes.data,
                                labels.ctypes.data, rmse.ctypes.data, winners.ctypes.data)
    msg = capi.lib().mi_last_error().decode()
    assert rc == capi.MI_ERR_INVALID_ARG and msg.startswith("mi_segment_plane:") and "null context" in msg
    assert (planes == -7).all() and (inl == -7).all() and (labels == -7).all() and (rmse == -7).all() and (winners == -7).all() and found.value == -7
    triples, valid, plane4, count = np.full(6, -7, np.int32), np.full(2, 7, np.uint8), np.full(8, -7, np.float32), np.full(2, -7, np.int32)
    rc = capi.segment_plane_hypotheses_raw(None, cloud.ctypes.data, 4, 0.1, 10, 0, None, 0.0, 0, 2, triples.ctypes.data, valid.ctypes.data,
                                           plane4.ctypes.data, count.ctypes.data)
    msg = capi.lib().mi_last_error().decode()
    assert rc == capi.MI_ERR_INVALID_ARG and msg.startswith("mi_segment_plane_hypotheses:") and "null context" in msg
    assert (triples == -7).all() and (valid == 7).all() and (plane4 == -7).all() and (count == -7).all()
    out = (C.c_double * 8)(*([-7.0] * 8))
    assert capi.lib().mi_segment_plane_times(None, out) == capi.MI_ERR_INVALID_ARG and list(out) == [-7.0] * 8
    assert capi.lib().mi_last_error().decode().startswith("mi_segment_plane_times")


def test_restatement_on_a_lattice_worked_by_hand():
    L = lattice3()                                                    # index = x + 3 y + 9 z
    below = np.nextafter(np.float32(1), np.float32(0))
    for layer, at_one in ((0, 18), (1, 27), (2, 18)):                 # three points of layer z: the plane (0, 0, 1, -z)
        tri = L[[9 * layer, 9 * layer + 1, 9 * layer + 3]]
        valid, plane = R.planes_through(tri[None])
        assert valid.tolist() == [True] and plane[0].tolist() == [0.0, 0.0, 1.0, -float(layer)]
        # threshold 1: the layer and its neighbours, whose points lie exactly AT the threshold; the float below 1: the layer alone
        assert R.counts(plane, valid, L, 1.0).tolist() == [at_one] and R.counts(plane, valid, L, below).tolist() == [9]
        mask = R.inlier_mask(plane[0], L, 1.0)[0]
        assert np.flatnonzero(mask).tolist() == [i for i in range(27) if abs(i // 9 - layer) <= 1]
    # the other orientation of the same three points: the normal is turned, the counts are not
    valid, plane = R.planes_through(L[[9, 12, 10]][None])
    assert plane[0].tolist() == [0.0, 0.0, -1.0, 1.0] and R.counts(plane, valid, L, 1.0).tolist() == [27]
    # a diagonal plane x + y + z = 3 through (1, 1, 1): 7 lattice points on it
    valid, plane = R.planes_through(L[[5, 7, 11]][None])              # (2, 1, 0), (1, 2, 0), (2, 0, 1)
    assert valid.all() and R.counts(plane, valid, L, 1e-3).tolist() == [7]
    # the whole call: the best plane of the lattice at threshold 1 holds all 27 points, whatever the draws
    ref = R.segment(L, 1.0, 50, seed=3, refine_iterations=0)
    assert ref["n_planes"] == 1 and ref["inliers"].tolist() == [27] and (ref["labels"] == 0).all()


def test_restatement_on_degenerate_clouds():
    line = np.array([[0, 0, 0], [1, 2, 3], [2, 4, 6]], np.float32)     # three collinear points
    valid, plane = R.planes_through(line[None])
    assert valid.tolist() == [False] and (plane == 0).all()
    for cloud in (line, np.linspace(0, 1, 50, dtype=np.float32)[:, None] * np.array([[1.0, 2.0, 4.0]], np.float32)):
        ref = R.segment(cloud, 0.5, 64, seed=1)
        assert ref["n_planes"] == 0 and (ref["labels"] == -1).all() and ref["planes"].shape == (0, 4)
    same = np.tile(np.array([[1.5, -2.25, 3.0]], np.float32), (200, 1))           # two hundred identical points
    ref = R.segment(same, 1e-3, 64, seed=1)
    assert ref["n_planes"] == 0 and (ref["labels"] == -1).all()
    _, valid, plane4 = R.hypotheses(same, np.arange(200), 1, 0, 64)
    assert not valid.any() and (plane4 == 0).all()


def test_restatement_recovers_an_integer_plane():
    g = np.arange(-3, 4)
    y, z = [a.ravel() for a in np.meshgrid(g, g, indexing="ij")]
    on = np.stack([9 - 2 * y - 2 * z, y, z], axis=1).astype(np.float32)           # x + 2 y + 2 z = 9 on 49 lattice points
    off = np.array([[0, 0, 0], [1, 1, 1], [-5, 2, 0], [3, 3, 3]], np.float32)
    cloud = np.concatenate([on, off])
    want = (np.array([1.0, 2.0, 2.0, -9.0]) / 3.0).astype(np.float32)
    for refine in (0, 2):
        ref = R.segment(cloud, 1e-3, 100, seed=5, refine_iterations=refine)
        assert ref["n_planes"] == 1 and ref["inliers"].tolist() == [49] and ref["labels"].tolist() == [0] * 49 + [-1] * 4
        plane = ref["planes"][0]
        sign = np.float32(1 if plane[0] > 0 else -1)
        if refine == 0:
            assert np.array_equal(sign * plane, want)                 # |N| = 3 k exactly: every triple gives the same bits
        else:
            assert np.abs(sign * plane - want).max() <= 2.0 ** -22
        assert ref["rmse"][0] <= 1e-6


def planted_three():
    """300, 200 and 100 points on the parallel planes z = 0, 5, 10 (float32 coordinates: exactly on them), handed over interleaved"""
    rng = np.random.default_rng(11)
    which = rng.permutation(np.repeat([0, 1, 2], [300, 200, 100]))
    cloud = np.concatenate([rng.uniform(-4, 4, (600, 2)), 5.0 * which[:, None]], axis=1).astype(np.float32)
    return cloud, which


def test_restatement_finds_three_planted_planes_in_descending_size():
    cloud, which = planted_three()
    ref = R.segment(cloud, 0.01, 200, seed=7, refine_iterations=2, max_planes=4, min_inliers=50)
    assert ref["n_planes"] == 3 and ref["inliers"].tolist() == [300, 200, 100] and np.array_equal(ref["labels"], which)
    for p in range(3):
        plane = ref["planes"][p].astype(np.float64)
        assert abs(abs(plane[2]) - 1) <= 1e-6 and abs(plane[3] / plane[2] + 5.0 * p) <= 1e-5
    # a higher bar than the third plane's size: two come back
    ref = R.segment(cloud, 0.01, 200, seed=7, max_planes=4, min_inliers=150)
    assert ref["n_planes"] == 2 and ref["inliers"].tolist() == [300, 200] and np.array_equal(ref["labels"], np.where(which == 2, -1, which))
    # max_planes = 1 stops behind the first
    ref = R.segment(cloud, 0.01, 200, seed=7, max_planes=1, min_inliers=50)
    assert ref["n_planes"] == 1 and np.array_equal(ref["labels"], np.where(which == 0, 0, -1))


def axis_case():
    """100 points on the horizontal plane z = 0 (x from 1) and 300 on the vertical plane x = 0 (z from 1), interleaved"""
    rng = np.random.default_rng(12)
    flat = np.stack([rng.uniform(1, 9, 100), rng.uniform(-4, 4, 100), np.zeros(100)], axis=1)
    wall = np.stack([np.zeros(300), rng.uniform(-4, 4, 300), rng.uniform(1, 9, 300)], axis=1)
    which = rng.permutation(np.repeat([0, 1], [100, 300]))
    cloud = np.empty((400, 3), np.float32)
    cloud[which == 0], cloud[which == 1] = flat, wall
    return cloud, which


def test_restatement_of_the_axis_rule():
    cloud, which = axis_case()
    ref = R.segment(cloud, 0.01, 300, seed=9, min_inliers=50)
    assert ref["n_planes"] == 1 and ref["inliers"].tolist() == [300] and np.array_equal(ref["labels"] == 0, which == 1)
    ref = R.segment(cloud, 0.01, 300, seed=9, min_inliers=50, axis=[0, 0, 2], min_axis_cosine=0.9)
    assert ref["n_planes"] == 1 and ref["inliers"].tolist() == [100] and np.array_equal(ref["labels"] == 0, which == 0)
    assert abs(abs(float(ref["planes"][0][2])) - 1) <= 1e-6
    # the rule itself: a normal 30 degrees off the axis passes cos 0.8 and fails cos 0.9, whatever the axis' length and sign
    tri = np.array([[0, 0, 0], [1, 0, 0], [0, np.sqrt(3) / 2, 0.5]], np.float32)
    for axis in ([0, 0, 1], [0, 0, -7.5]):
        assert R.planes_through(tri[None], axis, 0.8)[0].tolist() == [True] and R.planes_through(tri[None], axis, 0.9)[0].tolist() == [False]
