"""CPU suite: the clustering entry points exist, the argument errors that need no device are refused, the defaults are the documented
ones, and the restatement the GPU tests use as their oracle (tests/cluster_reference.py) gives the answers worked by hand on the
3 x 3 x 3 integer lattice of tests/test_knn_abi.py, a single point, identical points, two pairs of core points with a bridge between
them and three clusters under the size filter; where sklearn imports, its DBSCAN agrees on everything but the border labels."""
import ctypes as C

import numpy as np
import pytest

import cluster_reference as R
import knn_reference as K
from test_knn_abi import lattice3

MODES = [K.DIST_CPU_ROUNDING, K.DIST_FMA]


def test_library_exports_the_cluster_entry_points(capi):
    lib = capi.lib()
    for name in ("mi_cluster_dbscan", "mi_cluster_dbscan_times", "mi_cluster_params_default"):
        assert hasattr(lib, name), name
        assert name in capi.EXPORTS, name
    assert lib.mi_abi_version() == 4          # additive: no signature of version 4 changed
    assert C.sizeof(capi.ClusterParams) == 64


def test_a_null_context_is_refused_without_a_device(capi):
    cloud = np.zeros((4, 3), np.float32)
    labels, sizes, core, grouped = np.full(4, -7, np.int32), np.full(4, -7, np.int32), np.full(4, 7, np.uint8), np.full(4, -7, np.int32)
    n_clusters, n_grouped = C.c_int(-7), C.c_int(-7)
    p = capi.cluster_params(radius=1.0)
    rc = capi.cluster_dbscan_raw(None, cloud.ctypes.data, 4, C.addressof(p), labels.ctypes.data, C.addressof(n_clusters), sizes.ctypes.data, 4,
                                 core.ctypes.data, grouped.ctypes.data, C.addressof(n_grouped))
    msg = capi.lib().mi_last_error().decode()
    assert rc == capi.MI_ERR_INVALID_ARG and msg.startswith("mi_cluster_dbscan") and "null context" in msg
    assert (labels == -7).all() and (sizes == -7).all() and (core == 7).all() and (grouped == -7).all() and n_clusters.value == -7 and n_grouped.value == -7
    out = (C.c_double * 8)()
    f = capi.lib().mi_cluster_dbscan_times
    f.argtypes, f.restype = [C.c_void_p, C.c_void_p], C.c_int
    assert f(None, out) == capi.MI_ERR_INVALID_ARG


def test_defaults_are_the_documented_ones(capi):
    p = capi.cluster_params()
    assert p.radius == 0.0                                                     # the caller must set it
    assert (p.min_points, p.min_cluster_size, p.max_cluster_size, p.dist_mode) == (1, 1, 0, capi.DIST_CPU_ROUNDING) and list(p.reserved) == [0] * 11
    q = capi.cluster_params(radius=0.9, min_points=8, max_cluster_size=50, dist_mode=capi.DIST_FMA)
    assert (q.radius, q.min_points, q.min_cluster_size, q.max_cluster_size, q.dist_mode) == (float(np.float32(0.9)), 8, 1, 50, capi.DIST_FMA)
    with pytest.raises(AttributeError):
        capi.cluster_params(no_such_field=1)


def consistent(ref, n):
    """what every answer satisfies: sizes are the labels' histogram, grouped is the (label, index) order"""
    labels = ref["labels"]
    assert labels.shape == (n,) and labels.min() >= -1 and labels.max() == ref["n_clusters"] - 1
    assert np.array_equal(np.bincount(labels[labels >= 0], minlength=ref["n_clusters"]), ref["sizes"])
    assert np.array_equal(ref["grouped"], np.lexsort((np.arange(n), labels))[(labels < 0).sum():])
    return True


@pytest.mark.parametrize("mode", MODES)
def test_restatement_on_a_lattice_worked_by_hand(mode):
    L = lattice3()                                                    # index = x + 3 y + 9 z
    # radius 1: the face neighbours, all of them AT the radius -- 3 at a corner, 4 on an edge, 5 on a face, 6 at the centre
    for min_points in (1, 2, 4):                                      # every point is core: one cluster of 27
        ref = R.dbscan(L, 1.0, min_points, dist_mode=mode)
        assert ref["n_clusters"] == 1 and ref["sizes"].tolist() == [27] and (ref["labels"] == 0).all() and ref["is_core"].all() and consistent(ref, 27)
        assert ref["grouped"].tolist() == list(range(27))
    # min_points 7: only the centre (6 neighbours and itself) is core; its six face neighbours are border, the other 20 noise
    ref = R.dbscan(L, 1.0, 7, dist_mode=mode)
    faces = [4, 10, 12, 14, 16, 22]
    assert np.flatnonzero(ref["is_core"]).tolist() == [13] and ref["n_clusters"] == 1 and ref["sizes"].tolist() == [7]
    assert np.flatnonzero(ref["labels"] == 0).tolist() == sorted(faces + [13]) and (ref["labels"] < 0).sum() == 20 and consistent(ref, 27)
    # the float below 1: nobody has a neighbour
    below = np.nextafter(np.float32(1), np.float32(0))
    ref = R.dbscan(L, below, 1, dist_mode=mode)
    assert ref["n_clusters"] == 27 and ref["labels"].tolist() == list(range(27)) and (ref["sizes"] == 1).all() and ref["is_core"].all()
    ref = R.dbscan(L, below, 2, dist_mode=mode)
    assert ref["n_clusters"] == 0 and (ref["labels"] == -1).all() and not ref["is_core"].any() and len(ref["grouped"]) == 0 and len(ref["sizes"]) == 0


@pytest.mark.parametrize("mode", MODES)
def test_restatement_on_degenerate_clouds(mode):
    one = np.array([[1.5, -2.25, 3.0]], np.float32)
    ref = R.dbscan(one, 1.0, 1, dist_mode=mode)                       # a single point is a cluster of its own ...
    assert (ref["labels"].tolist(), ref["n_clusters"], ref["sizes"].tolist(), ref["is_core"].tolist(), ref["grouped"].tolist()) == ([0], 1, [1], [1], [0])
    ref = R.dbscan(one, 1.0, 2, dist_mode=mode)                       # ... or noise
    assert (ref["labels"].tolist(), ref["n_clusters"], ref["is_core"].tolist()) == ([-1], 0, [0])
    same = np.tile(one, (200, 1))                                     # identical points: every other one is a neighbour at d2 = +0
    for min_points in (1, 200):
        ref = R.dbscan(same, 1e-3, min_points, dist_mode=mode)
        assert ref["n_clusters"] == 1 and ref["sizes"].tolist() == [200] and (ref["labels"] == 0).all() and ref["is_core"].all()
    assert R.dbscan(same, 1e-3, 201, dist_mode=mode)["n_clusters"] == 0


def bridge_case(near_x):
    """Two pairs of core points and, between them, one point that is not core and a neighbour of all four (radius 1, min_points 6).  Every
    pair has three satellites out of the bridge's reach, so a pair point has 5 neighbours (its partner, the bridge, the satellites: core), a
    satellite 4 (the pair, the other two: border) and the bridge 4.  Indices: the pair at x = +0.9 and its satellites 0 .. 4, the bridge 5,
    the pair at x = -near_x and its satellites 6 .. 10."""
    def side(x, sign):
        return [[x, 0.3, 0], [x, -0.3, 0], [sign * 1.6, 0, 0], [sign * 1.6, 0, 0.3], [sign * 1.6, 0, -0.3]]
    return np.array(side(0.9, 1.0) + [[0, 0, 0]] + side(-near_x, -1.0), np.float32)


@pytest.mark.parametrize("mode", MODES)
def test_restatement_keeps_two_pairs_apart_across_a_bridge(mode):
    # an exact tie (the differences negate exactly): the bridge goes with the lowest index among the four, point 0
    ref = R.dbscan(bridge_case(0.9), 1.0, 6, dist_mode=mode)
    assert np.flatnonzero(ref["is_core"]).tolist() == [0, 1, 6, 7] and ref["n_clusters"] == 2
    assert ref["labels"].tolist() == [0] * 6 + [1] * 5 and ref["sizes"].tolist() == [6, 5] and consistent(ref, 11)
    # the other pair nearer: the bridge goes there, whatever the indices
    ref = R.dbscan(bridge_case(0.8), 1.0, 6, dist_mode=mode)
    assert np.flatnonzero(ref["is_core"]).tolist() == [0, 1, 6, 7] and ref["n_clusters"] == 2
    assert ref["labels"].tolist() == [0] * 5 + [1] * 6 and ref["sizes"].tolist() == [5, 6] and consistent(ref, 11)
    # with the bridge core as well (min_points 5) everything is one cluster
    ref = R.dbscan(bridge_case(0.9), 1.0, 5, dist_mode=mode)
    assert ref["n_clusters"] == 1 and ref["sizes"].tolist() == [11]


def filter_case():
    """three clusters along x, 10 apart, of 5, 2 and 4 points 0.5 apart, handed over interleaved: the smallest indices are 0, 1 and 2"""
    pts = [(10.0 * c + 0.5 * k, 0.0, 0.0, c) for c, size in enumerate((5, 2, 4)) for k in range(size)]
    pts.sort(key=lambda p: (p[0] - 10.0 * p[3], p[3]))
    return np.array([p[:3] for p in pts], np.float32), np.array([p[3] for p in pts])


@pytest.mark.parametrize("mode", MODES)
def test_restatement_of_the_size_filter_and_the_numbering(mode):
    cloud, which = filter_case()
    ref = R.dbscan(cloud, 0.6, 1, dist_mode=mode)
    assert ref["n_clusters"] == 3 and ref["sizes"].tolist() == [5, 2, 4] and ref["labels"].tolist() == which.tolist()
    ref = R.dbscan(cloud, 0.6, 1, min_cluster_size=3, dist_mode=mode)             # the middle one goes and the numbering closes the gap
    assert ref["n_clusters"] == 2 and ref["sizes"].tolist() == [5, 4] and ref["labels"].tolist() == [{0: 0, 1: -1, 2: 1}[c] for c in which]
    assert ref["is_core"].all() and consistent(ref, 11)
    ref = R.dbscan(cloud, 0.6, 1, max_cluster_size=4, dist_mode=mode)             # the first one goes
    assert ref["n_clusters"] == 2 and ref["sizes"].tolist() == [2, 4] and ref["labels"].tolist() == [{0: -1, 1: 0, 2: 1}[c] for c in which]
    ref = R.dbscan(cloud, 0.6, 1, min_cluster_size=3, max_cluster_size=4, dist_mode=mode)
    assert ref["n_clusters"] == 1 and ref["sizes"].tolist() == [4] and ref["grouped"].tolist() == np.flatnonzero(which == 2).tolist()
    assert R.dbscan(cloud, 0.6, 1, min_cluster_size=6, dist_mode=mode)["n_clusters"] == 0


@pytest.mark.parametrize("min_points", (1, 4, 9))
def test_restatement_against_sklearn(min_points):
    cluster = pytest.importorskip("sklearn.cluster")
    spatial = pytest.importorskip("scipy.spatial")
    rng = np.random.default_rng(41)
    centres = rng.uniform(-6, 6, (4, 3))
    cloud = np.concatenate([c + 0.5 * rng.normal(size=(150, 3)) for c in centres] + [rng.uniform(-8, 8, (150, 3))]).astype(np.float32)
    radius = 0.45
    gap = np.abs(spatial.distance.pdist(cloud.astype(np.float64)) - float(np.float32(radius))).min()
    # no pair near the radius, so float32 and float64 see one neighbour graph: a float32 d2 carries three roundings of the squares' sum and one
    # of each difference, under 6 * 2^-24 of itself, so its root is within 3 * 2^-24 r = 8e-8 of the float64 distance
    assert gap > 1e-6
    theirs = cluster.DBSCAN(eps=float(np.float32(radius)), min_samples=min_points, algorithm="brute").fit(cloud.astype(np.float64))
    for mode in MODES:
        ref = R.dbscan(cloud, radius, min_points, dist_mode=mode)
        core = np.flatnonzero(ref["is_core"])
        assert np.array_equal(core, np.sort(theirs.core_sample_indices_))
        assert np.array_equal(ref["raw"] < 0, theirs.labels_ < 0)     # the noise set
        # the partition of the core points, up to renaming: the pairs (ours, theirs) are a bijection
        pairs = set(zip(ref["raw"][core].tolist(), theirs.labels_[core].tolist()))
        assert len(pairs) == len({a for a, _ in pairs}) == len({b for _, b in pairs})
        assert ref["n_clusters"] == len(pairs) >= 4
