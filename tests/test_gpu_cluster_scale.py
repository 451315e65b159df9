"""GPU suite of mi_cluster_dbscan beyond the 5 000 points of tests/test_gpu_cluster.py, against the restatement that scales
(tests/cluster_reference.py: the binned pair list, scipy's components; held equal to the distance matrix's and the Python union-find's by
tests/test_cluster_scale_reference.py).  The cases: tests/cluster_scale_cases.py; that each reaches the regime it is named for: the same
CPU file.  As in the small suite every comparison is equality, element for element and dtype for dtype, in both distance arithmetics:
labels, n_clusters, cluster_sizes, is_core and grouped_index.  No tolerance exists here.

What runs here and nowhere else:
  the grouping's 20-bit sort    thinned (thousands of clusters), scene at min_points 1, the chain below radius 1 (10^5 clusters)
  the grouping's 30-bit sort    singletons below radius 1: 2^20 + 1 clusters.  The branch beyond it, found > 2^30 with its second sort,
                                cannot be reached by a cloud that fits and stays untested
  sets of 10^5 and 10^6 points  thinned's giant, the chains, singletons at radius 1 (16 385 workgroups hooking into one set)
  the deepest parent list       the chain in ascending index order: every lane hooks under its predecessor
  more than 256 tiles           singletons: 1025 tiles in both compactions
  a clamped axis                the chains: 1023 x 1 x 1 cells whose edge is the floor
  64 and more cells per axis    the scene at a quarter point per cell (79 per axis); singletons at the radius rule's own plan (102)
  ties between clusters         thinned: thousands of border points whose nearest core neighbours lie in different clusters at d2 = 1

Every call prints one line -- n, clusters, largest set, stage times -- so that a run's log (pytest -s) records what each case cost."""
import ctypes as C

import numpy as np
import pytest

import cluster_scale_cases as S
from test_gpu_cluster import check, reference as small_reference, clouds as small_clouds, run

pytestmark = pytest.mark.gpu

MODES = S.MODES


def timed(ctx, capi, what, cloud, **kw):
    """run() of the small suite, and the call's line for the log: the whole call as it ran, and the stages of a second, profiled call (the
    stream drained after each stage, so that a stage's time is its kernels'), which has to give the same bytes"""
    got = run(ctx, capi, cloud, **kw)
    whole = ctx.cluster_dbscan_times()["total"]
    ctx.profile_enable(True)
    try:
        again = run(ctx, capi, cloud, **kw)
        ms = ctx.cluster_dbscan_times()
    finally:
        ctx.profile_enable(False)
    assert again["n_clusters"] == got["n_clusters"] and all(again[k].tobytes() == got[k].tobytes() for k in got if k != "n_clusters"), what
    print("CLUSTER %s: n %d, clusters %d, largest %s, whole call %.3f ms; profiled: %s" % (
        what, len(cloud), got["n_clusters"], got["sizes"].max() if len(got["sizes"]) else "-", whole, " ".join("%s %.3f" % kv for kv in ms.items())))
    return got


# ---- 1. thinned: the 20-bit sort, a giant set, ties between clusters
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("min_points,min_size,max_size", S.THINNED_RUNS)
def test_thinned_lattice(ctx, capi, min_points, min_size, max_size, mode):
    ref = S.reference("thinned", S.THINNED_RADIUS, min_points, min_size, max_size, mode)
    what = "thinned %d [%d, %d] mode %d" % (min_points, min_size, max_size, mode)
    assert S.sort_bits(ref["n_clusters"]) == 20, what
    check(timed(ctx, capi, what, S.cloud("thinned"), radius=S.THINNED_RADIUS, min_points=min_points, min_cluster_size=min_size, max_cluster_size=max_size,
                dist_mode=mode), ref, what)


@pytest.mark.parametrize("mode", MODES)
def test_thinned_ties_between_clusters(ctx, capi, mode):
    """the border points whose nearest core neighbours lie in different clusters, named: each takes the cluster of the LOWEST such index"""
    ref = S.reference("thinned", S.THINNED_RADIUS, S.THINNED_MIN_POINTS, 1, 0, mode)
    tied = S.tied_borders(S.pairs("thinned", S.THINNED_RADIUS, mode), ref)
    assert len(tied) >= 1000
    got = run(ctx, capi, S.cloud("thinned"), want=(), radius=S.THINNED_RADIUS, min_points=S.THINNED_MIN_POINTS, dist_mode=mode)
    wrong = np.flatnonzero(got["labels"][tied] != ref["labels"][tied])
    assert wrong.size == 0, "%d of %d tied border points in another cluster, first point %d: got %d, want %d" % (
        wrong.size, len(tied), tied[wrong[0]], got["labels"][tied[wrong[0]]], ref["labels"][tied[wrong[0]]])


@pytest.mark.parametrize("mode", MODES)
def test_thinned_optional_outputs(ctx, capi, mode):
    cloud = S.cloud("thinned")
    ref = S.reference("thinned", S.THINNED_RADIUS, S.THINNED_MIN_POINTS, 1, 0, mode)
    n, nc = len(cloud), ref["n_clusters"]
    fields = dict(radius=S.THINNED_RADIUS, min_points=S.THINNED_MIN_POINTS, dist_mode=mode)
    check(run(ctx, capi, cloud, want=(), **fields), ref, "labels alone")
    # a cluster_cap below n_clusters, both above 1024: the first cluster_cap sizes, the sentinel behind them; n_grouped without grouped_index
    cap = 1500
    assert nc > cap > 1024
    labels, sizes, n_clusters, n_grouped = np.empty(n, np.int32), np.full(nc, -7, np.int32), C.c_int(-7), C.c_int(-7)
    p = capi.cluster_params(**fields)
    rc = capi.cluster_dbscan_raw(ctx._h, cloud.ctypes.data, n, C.addressof(p), labels.ctypes.data, C.addressof(n_clusters), sizes.ctypes.data, cap, None, None,
                                 C.addressof(n_grouped))
    assert rc == capi.MI_OK and n_clusters.value == nc and n_grouped.value == len(ref["grouped"]) and np.array_equal(labels, ref["labels"])
    assert np.array_equal(sizes[:cap], ref["sizes"][:cap]) and (sizes[cap:] == -7).all()


# ---- 2. the scene: generic positions, the two arithmetics differ in their last bit
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("min_points", S.SCENE_MIN_POINTS)
def test_scene(ctx, capi, min_points, mode):
    ref = S.reference("scene", S.SCENE_RADIUS, min_points, 1, 0, mode)
    what = "scene %d mode %d" % (min_points, mode)
    check(timed(ctx, capi, what, S.cloud("scene"), radius=S.SCENE_RADIUS, min_points=min_points, dist_mode=mode), ref, what)


@pytest.mark.parametrize("mode", MODES)
def test_scene_at_64_and_more_cells_per_axis(capi, monkeypatch, mode):
    """the same answer from a grid of 79 cells per axis (a quarter point per cell), where the radius rule's own plan has 50"""
    monkeypatch.setenv("MISLAM_KNN_POINTS_PER_CELL", S.SCENE_FINE_PPC)
    ref = S.reference("scene", S.SCENE_RADIUS, 5, 1, 0, mode)
    with capi.Context(0) as c2:
        check(timed(c2, capi, "scene 5 mode %d, fine grid" % mode, S.cloud("scene"), radius=S.SCENE_RADIUS, min_points=5, dist_mode=mode), ref, "fine grid")


# ---- 3. the long chain: the deepest parent list, a clamped axis
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("order", S.CHAIN_ORDERS)
def test_long_chain(ctx, capi, order, mode):
    cloud = S.cloud("chain " + order)
    for radius, min_points in S.CHAIN_RUNS:
        ref = S.reference("chain " + order, radius, min_points, 1, 0, mode)
        what = "chain %s radius %.8g min_points %d mode %d" % (order, radius, min_points, mode)
        check(timed(ctx, capi, what, cloud, radius=radius, min_points=min_points, dist_mode=mode), ref, what)


# ---- 4. singletons: the 30-bit sort, 1025 tiles, a set of 2^20 + 1 points
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("together", [False, True], ids=["alone", "one set"])
def test_singletons(ctx, capi, together, mode):
    cloud = S.cloud("singletons")
    n = len(cloud)
    assert n > 1 << 20 and S.sort_bits(n) == 30 and S.compact_tiles(n) > 256
    what = "singletons %s mode %d" % ("one set" if together else "alone", mode)
    check(timed(ctx, capi, what, cloud, radius=1.0 if together else S.BELOW_ONE, dist_mode=mode), S.prefix_answer(n, together), what)


# ---- 5. state
@pytest.mark.parametrize("mode", MODES)
def test_the_same_call_twice_with_the_long_chain_between(ctx, capi, mode):
    fields = dict(radius=S.THINNED_RADIUS, min_points=S.THINNED_MIN_POINTS, dist_mode=mode)
    a = run(ctx, capi, S.cloud("thinned"), **fields)
    run(ctx, capi, S.cloud("chain ascending"), radius=1.0, dist_mode=mode)
    b = run(ctx, capi, S.cloud("thinned"), **fields)
    assert a["n_clusters"] == b["n_clusters"] and all(a[k].tobytes() == b[k].tobytes() for k in ("labels", "sizes", "is_core", "grouped"))


@pytest.mark.parametrize("mode", MODES)
def test_a_small_cloud_after_the_large_ones(ctx, capi, mode):
    """the context's buffers have grown to 2^20 + 1 points and now serve 1 025: the small suite's case still equals its restatement"""
    big = S.cloud("singletons")
    check(run(ctx, capi, big, radius=S.BELOW_ONE, dist_mode=mode), S.prefix_answer(len(big), False), "the large call")
    check(run(ctx, capi, small_clouds()["blobs"][:1025], radius=0.6, min_points=4, dist_mode=mode), small_reference("blobs", 1025, 0.6, 4, 1, 0, mode), "after the large call")


def test_a_context_destroyed_after_a_large_call_leaves_no_device_buffer_behind(capi, ctx):
    big = S.cloud("singletons")
    start = capi.selftest_live_buffers()
    with capi.Context(0) as c2:
        check(run(c2, capi, big, radius=1.0), S.prefix_answer(len(big), True), "the large call")
        assert capi.selftest_live_buffers() > start
    assert capi.selftest_live_buffers() == start
