"""What tests/test_gpu_cluster_scale.py rests on, held here with no device: the binned pair list of tests/cluster_reference.py is the
distance matrix's, all four arrays in order, and scipy's components give the Python union-find's answer -- on every cloud of
tests/test_gpu_cluster.py at that suite's radii, on the hand-worked small clouds and on prefixes of the large ones, in both arithmetics;
the analytic answers of the raster prefix are dbscan()'s on a small instance of the same construction; and every case of
tests/cluster_scale_cases.py reaches the regime it is named for, by its restatement and the restated grid plan alone.  If a seed, a
share or one of the plan's constants changes, this says which case no longer tests what it claims."""
import numpy as np
import pytest

import cluster_reference as R
import cluster_scale_cases as C
import knn_reference as K
from test_gpu_cluster import BLOB_RADIUS, clouds
from test_knn_abi import lattice3

PREFIX = 3000
SMALL_SIDE, SMALL_PREFIX = 9, 600
# 3 000 of a large cloud's points are 3.4 times as far apart as all of them: the radii grow with that.  On the lattice, 5 is a radius with
# many points exactly AT it, (5, 0, 0) and (3, 4, 0)
THINNED_PREFIX_RADIUS, SCENE_PREFIX_RADIUS = 5.0, 4 * C.SCENE_RADIUS


def small_cases():
    """(name, cloud, radius): every cloud of tests/test_gpu_cluster.py at its radii, the small exact clouds, prefixes of the large ones"""
    small = clouds()
    same = np.tile(np.array([[1.5, -2.25, 3.0]], np.float32), (200, 1))
    return [("blobs", small["blobs"], BLOB_RADIUS), ("blobs wide", small["blobs"], 0.6), ("ball", small["ball"], 0.25),
            ("chain", small["chain"], 1.0), ("chain below 1", small["chain"], C.BELOW_ONE), ("straggler", small["straggler"], 0.6),
            ("lattice3", lattice3(), 1.0), ("lattice3 below 1", lattice3(), C.BELOW_ONE), ("identical", same, 1e-3),
            ("thinned prefix", C.cloud("thinned")[:PREFIX], THINNED_PREFIX_RADIUS), ("scene prefix", C.cloud("scene")[:PREFIX], SCENE_PREFIX_RADIUS),
            ("raster prefix", C.raster_prefix(SMALL_SIDE, SMALL_PREFIX, 3), 1.0)]


CASES = ("blobs", "blobs wide", "ball", "chain", "chain below 1", "straggler", "lattice3", "lattice3 below 1", "identical", "thinned prefix",
         "scene prefix", "raster prefix")


def test_d2_pairs_is_d2_matrix_element_for_element():
    rng = np.random.default_rng(41)
    q, c = rng.normal(size=(300, 3)).astype(np.float32), (rng.normal(size=(400, 3)) * [1, 10, 1000]).astype(np.float32)
    c[:50] = q[:50]                                                   # zeros, and differences far below the coordinates
    c[50:100] = np.nextafter(q[50:100], np.float32(np.inf))
    i, j = np.divmod(np.arange(300 * 400), 400)
    differ = 0
    for mode in C.MODES:
        want = K.d2_matrix(q, c, mode)
        got = K.d2_pairs(q[i], c[j], mode)
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.ravel().view(np.uint32)), mode
        differ += int((want.view(np.uint32) != K.d2_matrix(q, c, K.DIST_CPU_ROUNDING).view(np.uint32)).sum())
    assert differ > 1000                                              # (the two arithmetics are told apart by this input)


@pytest.mark.parametrize("mode", C.MODES)
@pytest.mark.parametrize("name", CASES)
def test_the_binned_pairs_are_the_distance_matrix_pairs(name, mode):
    cloud, radius = next((c, r) for what, c, r in small_cases() if what == name)
    want, got = R.neighbour_pairs(cloud, radius, mode), R.neighbour_pairs_binned(cloud, radius, mode)
    assert got[0] == want[0] == len(cloud)
    for a, b, what in zip(got[1:], want[1:], ("i", "j", "key")):
        assert a.dtype == b.dtype and np.array_equal(a, b), (name, what)
    if name not in ("chain below 1", "lattice3 below 1"):
        assert len(want[1]) > 0, name                                 # (not vacuous)
    # scipy's components against the Python union-find, with and without border points and with a size filter
    for min_points, lo, hi in ((1, 1, 0), (4, 1, 0), (5, 3, 500)):
        a = R.dbscan(cloud, radius, min_points, lo, hi, mode, pairs=want)
        b = R.dbscan(cloud, radius, min_points, lo, hi, mode, pairs=got, components="scipy")
        assert a["n_clusters"] == b["n_clusters"], (name, min_points)
        for key in ("raw", "labels", "sizes", "is_core", "grouped"):
            assert a[key].dtype == b[key].dtype and np.array_equal(a[key], b[key]), (name, min_points, key)


def test_the_prefixes_are_not_degenerate():
    for name in ("thinned prefix", "scene prefix"):
        cloud, radius = next((c, r) for what, c, r in small_cases() if what == name)
        ref = R.dbscan(cloud, radius, 4, pairs=R.neighbour_pairs_binned(cloud, radius))
        border = (ref["is_core"] == 0) & (ref["raw"] >= 0)
        assert ref["n_clusters"] >= 3 and border.sum() > 0 and (ref["raw"] < 0).sum() > 0, name


def test_the_binned_pairs_where_the_box_asks_for_more_bins_than_fit():
    """a far straggler at a small radius: the edge grows to box / BIN_MAX_DIM, and a coarser bin is a superset still"""
    cloud = np.concatenate([clouds()["blobs"][:400], np.array([[9e6, -7e6, 8e6]], np.float32)])
    assert 9e6 / 0.35 > R.BIN_MAX_DIM
    for mode in C.MODES:
        for a, b in zip(R.neighbour_pairs_binned(cloud, 0.35, mode)[1:], R.neighbour_pairs(cloud, 0.35, mode)[1:]):
            assert len(a) > 100 and np.array_equal(a, b)


def test_the_raster_prefix_has_the_analytic_answers():
    cloud = C.raster_prefix(SMALL_SIDE, SMALL_PREFIX, 3)
    assert cloud.shape == (SMALL_PREFIX, 3) and SMALL_PREFIX % SMALL_SIDE != 0 and SMALL_PREFIX > SMALL_SIDE ** 2     # layers, rows, a partial row
    for mode in C.MODES:
        for radius, together in ((1.0, True), (C.BELOW_ONE, False)):
            ref, want = R.dbscan(cloud, radius, 1, dist_mode=mode), C.prefix_answer(SMALL_PREFIX, together)
            assert ref["n_clusters"] == want["n_clusters"]
            for key in ("labels", "sizes", "is_core", "grouped"):
                assert ref[key].dtype == want[key].dtype and np.array_equal(ref[key], want[key]), (radius, key)
    # the large instance is the same construction: the first n sites in raster order, each once, in another order
    big = C.cloud("singletons")
    side = C.SINGLETONS_SIDE
    site = (big[:, 0] + side * big[:, 1] + side * side * big[:, 2].astype(np.float64)).astype(np.int64)
    assert np.array_equal(np.sort(site), np.arange(C.SINGLETONS_POINTS)) and not np.array_equal(site, np.arange(C.SINGLETONS_POINTS))


def test_cases_reach_the_regimes_they_are_named_for():
    mode = K.DIST_CPU_ROUNDING
    # ---- thinned: the 20-bit sort, a giant set, ties between clusters, noise; a filter that bites
    thinned = C.cloud("thinned")
    assert len(thinned) > 100_000 and np.array_equal(thinned, np.round(thinned)) and thinned.max() < 2 ** 10       # small integers: d2 is exact
    free = C.reference("thinned", C.THINNED_RADIUS, C.THINNED_MIN_POINTS, 1, 0, mode)
    assert 1024 < free["n_clusters"] <= 1 << 20 and C.sort_bits(free["n_clusters"]) == 20
    assert free["sizes"].max() > 40_000 and (free["labels"] < 0).sum() > 0
    tied = C.tied_borders(C.pairs("thinned", C.THINNED_RADIUS, mode), free)
    assert len(tied) >= 1000 and (free["is_core"][tied] == 0).all() and (free["labels"][tied] >= 0).all()
    for other in C.MODES:                                             # (exact distances: one pair list, bit for bit, in both arithmetics)
        for a, b in zip(C.pairs("thinned", C.THINNED_RADIUS, other)[1:], C.pairs("thinned", C.THINNED_RADIUS, mode)[1:]):
            assert np.array_equal(a, b)
    assert C.THINNED_RUNS[0] == (C.THINNED_MIN_POINTS, 1, 0)
    every_core = C.reference("thinned", C.THINNED_RADIUS, *C.THINNED_RUNS[1], mode)
    assert C.THINNED_RUNS[1][0] == 1 and every_core["is_core"].all() and every_core["n_clusters"] > free["n_clusters"]
    assert C.sort_bits(every_core["n_clusters"]) == 20 and every_core["sizes"].max() > 100_000 and (every_core["sizes"] == 1).sum() > 1000
    filtered = C.reference("thinned", C.THINNED_RADIUS, *C.THINNED_RUNS[2], mode)
    lo, hi = C.THINNED_RUNS[2][1:]
    assert 1 <= filtered["n_clusters"] < free["n_clusters"] and C.sort_bits(filtered["n_clusters"]) == 20
    assert free["sizes"].max() > hi and free["sizes"].min() < lo and np.array_equal(filtered["is_core"], free["is_core"])

    # ---- scene: generic positions; the two arithmetics differ; the 10-bit sort at this size; border and noise; a fine grid
    scene = C.cloud("scene")
    assert scene.shape == (C.SCENE_POINTS, 3) and scene.dtype == np.float32
    keys = [C.pairs("scene", C.SCENE_RADIUS, m)[3] for m in C.MODES]
    assert len(keys[0]) > 1_000_000 and (len(keys[0]) != len(keys[1]) or (keys[0] != keys[1]).sum() > 1000)
    runs = {mp: C.reference("scene", C.SCENE_RADIUS, mp, 1, 0, mode) for mp in C.SCENE_MIN_POINTS}
    assert min(C.sort_bits(r["n_clusters"]) for r in runs.values()) == 10 and max(C.sort_bits(r["n_clusters"]) for r in runs.values()) == 20
    at5 = runs[5]
    assert ((at5["is_core"] == 0) & (at5["labels"] >= 0)).sum() > 1000 and (at5["labels"] < 0).sum() > 1000 and at5["n_clusters"] >= 36
    assert len(C.tied_borders(C.pairs("scene", C.SCENE_RADIUS, mode), at5)) == 0      # (generic positions: the distance half decides alone)
    dims, _, raised = C.plan(scene, C.SCENE_RADIUS, C.SCENE_FINE_PPC)
    assert (dims >= 64).all() and (dims <= C.S.GRID_MAX_DIM).all() and not raised, dims
    assert (C.plan(scene, C.SCENE_RADIUS)[0] < 64).all()              # (the radius rule's own plan stops at one point per cell: hence the run above)

    # ---- long_chain: a raised, clamped x axis with y and z of one cell; one set of everything, in three index orders
    for order in C.CHAIN_ORDERS:
        chain = C.cloud("chain " + order)
        assert chain.shape == (C.CHAIN_POINTS, 3) and np.array_equal(np.sort(chain[:, 0]), np.arange(C.CHAIN_POINTS)) and not chain[:, 1:].any()
        for radius, _ in C.CHAIN_RUNS:
            dims, _, raised = C.plan(chain, radius)
            assert raised and dims[0] >= 1000 and dims[0] <= C.S.GRID_MAX_DIM and dims[1] == dims[2] == 1, (order, dims)
    assert (np.diff(C.cloud("chain ascending")[:, 0]) == 1).all() and (np.diff(C.cloud("chain descending")[:, 0]) == -1).all()
    assert (np.abs(np.diff(C.cloud("chain shuffled")[:, 0])) > 1).mean() > 0.99
    for order in C.CHAIN_ORDERS:
        one, ends, alone = (C.reference("chain " + order, radius, mp, 1, 0, mode) for radius, mp in C.CHAIN_RUNS)
        assert one["sizes"].tolist() == [C.CHAIN_POINTS] and one["is_core"].all()
        assert ends["sizes"].tolist() == [C.CHAIN_POINTS] and ends["is_core"].sum() == C.CHAIN_POINTS - 2
        assert alone["n_clusters"] == C.CHAIN_POINTS and C.sort_bits(alone["n_clusters"]) == 20          # 10^5 roots, one point each

    # ---- singletons: the 30-bit sort; more than 256 compaction tiles; 60 and more cells per axis at the radius rule's own plan
    n = C.SINGLETONS_POINTS
    assert len(C.cloud("singletons")) == n > 1 << 20 and C.sort_bits(n) == 30 and C.sort_bits(1 << 20) == 20
    assert C.compact_tiles(n) > 256
    assert all(C.compact_tiles(len(C.cloud(name))) <= 256 for name in ("thinned", "scene", "chain ascending"))      # (as the head of the cases says)
    for radius in (1.0, C.BELOW_ONE):
        dims, _, raised = C.plan(C.cloud("singletons"), radius)
        assert (dims >= 60).all() and not raised, dims
