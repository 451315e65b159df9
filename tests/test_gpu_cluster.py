"""GPU suite of mi_cluster_dbscan against the restatement of tests/cluster_reference.py.  The result is a pure integer function of the
input and the restatement's distances are the device's bit for bit, so every comparison is equality, element for element: labels,
n_clusters, cluster_sizes, is_core, grouped_index and n_grouped.  Every case runs in both distance arithmetics.  The restatement of a
cloud is built once per parameter set (lru_cache) and shared, unchanged, by every test that needs it."""
import ctypes as C
import functools

import numpy as np
import pytest

import cluster_reference as R
import knn_reference as K
from test_cluster_abi import bridge_case, filter_case
from test_knn_abi import lattice3

pytestmark = pytest.mark.gpu

MODES = (K.DIST_CPU_ROUNDING, K.DIST_FMA)
BELOW_ONE = float(np.nextafter(np.float32(1), np.float32(0)))
BLOB_RADIUS = 0.35


def frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def clouds():
    rng = np.random.default_rng(23)
    centres = np.array([[-4, -4, -3], [4, -3, 2], [0, 4, -2], [-3, 3, 4], [3, 3, -4]], np.float64)
    spread = (0.5, 0.7, 0.9, 0.6, 0.8)
    blobs = np.concatenate([c + s * rng.normal(size=(900, 3)) for c, s in zip(centres, spread)] + [rng.uniform(-7, 7, (500, 3))])
    blobs = blobs[rng.permutation(len(blobs))].astype(np.float32)             # 5 000 points: five Gaussian blobs and uniform noise, mixed
    ball = rng.normal(size=(4000, 3))
    ball = (ball / np.linalg.norm(ball, axis=1, keepdims=True) * rng.uniform(0, 1, (4000, 1)) ** (1 / 3)).astype(np.float32)
    chain = np.zeros((300, 3), np.float32)
    chain[:, 0] = rng.permutation(300)                                        # one apart along x, in a shuffled index order
    straggler = np.concatenate([blobs[:600], np.array([[9000.0, -7000.0, 8000.0]], np.float32)])
    return {"blobs": frozen(blobs), "ball": frozen(ball), "chain": frozen(chain), "straggler": frozen(straggler)}


@functools.lru_cache(maxsize=None)
def pairs(name, n, radius, mode):
    """the neighbour pairs of a main cloud (its first n points; 0: all): one pass over the distance matrix for every min_points and size filter"""
    return tuple(v if isinstance(v, int) else frozen(v) for v in R.neighbour_pairs(clouds()[name][:n] if n else clouds()[name], radius, mode))


@functools.lru_cache(maxsize=None)
def reference(name, n, radius, min_points, min_size, max_size, mode):
    cloud = clouds()[name][:n] if n else clouds()[name]
    ref = R.dbscan(cloud, radius, min_points, min_size, max_size, mode, pairs=pairs(name, n, radius, mode))
    return {k: (frozen(v) if isinstance(v, np.ndarray) else v) for k, v in ref.items()}


def run(ctx, capi, cloud, want=("sizes", "core", "grouped"), **fields):
    res = list(ctx.cluster_dbscan(cloud, capi.cluster_params(**fields), **{"want_" + name: name in want for name in ("sizes", "core", "grouped")}))
    out = {"labels": res.pop(0), "n_clusters": res.pop(0)}
    for name, key in (("sizes", "sizes"), ("core", "is_core"), ("grouped", "grouped")):
        if name in want:
            out[key] = res.pop(0)
    return out


def check(got, ref, what):
    assert got["n_clusters"] == ref["n_clusters"], what
    for key in ("labels", "sizes", "is_core", "grouped"):
        if key in got:
            assert got[key].dtype == ref[key].dtype and np.array_equal(got[key], ref[key]), (what, key)


def check_case(ctx, capi, cloud, what, **fields):
    """both arithmetics against a restatement made on the spot (the small cases)"""
    for mode in MODES:
        ref = R.dbscan(cloud, fields["radius"], fields.get("min_points", 1), fields.get("min_cluster_size", 1), fields.get("max_cluster_size", 0), mode)
        check(run(ctx, capi, cloud, dist_mode=mode, **fields), ref, "%s mode %d" % (what, mode))
    return ref


# ---- 1. the smallest clouds
def test_one_point_and_two_points(ctx, capi):
    one = np.array([[1.5, -2.25, 3.0]], np.float32)
    assert check_case(ctx, capi, one, "n = 1", radius=1.0)["labels"].tolist() == [0]
    assert check_case(ctx, capi, one, "n = 1, min_points 2", radius=1.0, min_points=2)["labels"].tolist() == [-1]
    above = float(np.nextafter(np.float32(3), np.float32(4)))
    for far, together in ((3.0, True), (above, False)):                       # exactly at the radius, and the float above it
        two = np.array([[0, 0, 0], [far, 0, 0]], np.float32)
        assert check_case(ctx, capi, two, "n = 2 at %r" % far, radius=3.0)["n_clusters"] == (1 if together else 2)
        assert check_case(ctx, capi, two, "n = 2 at %r, min_points 2" % far, radius=3.0, min_points=2)["n_clusters"] == (1 if together else 0)


def test_the_lattice_worked_by_hand(ctx, capi):
    L = lattice3()
    for min_points in (1, 4):
        assert check_case(ctx, capi, L, "lattice %d" % min_points, radius=1.0, min_points=min_points)["sizes"].tolist() == [27]
    ref = check_case(ctx, capi, L, "lattice 7", radius=1.0, min_points=7)
    assert ref["sizes"].tolist() == [7] and (ref["labels"] < 0).sum() == 20
    assert check_case(ctx, capi, L, "lattice below 1", radius=BELOW_ONE)["n_clusters"] == 27
    assert check_case(ctx, capi, L, "lattice below 1, min_points 2", radius=BELOW_ONE, min_points=2)["n_clusters"] == 0


def test_identical_points(ctx, capi):
    same = np.tile(np.array([[1.5, -2.25, 3.0]], np.float32), (200, 1))
    for min_points in (1, 200, 201):
        assert check_case(ctx, capi, same, "identical %d" % min_points, radius=1e-3, min_points=min_points)["n_clusters"] == (0 if min_points == 201 else 1)


def test_two_pairs_and_a_bridge(ctx, capi):
    assert check_case(ctx, capi, bridge_case(0.9), "bridge, tie", radius=1.0, min_points=6)["labels"].tolist() == [0] * 6 + [1] * 5
    assert check_case(ctx, capi, bridge_case(0.8), "bridge, nearer", radius=1.0, min_points=6)["labels"].tolist() == [0] * 5 + [1] * 6


# ---- 2. the union-find under load
@pytest.mark.parametrize("mode", MODES)
def test_a_shuffled_chain_is_one_component(ctx, capi, mode):
    chain = clouds()["chain"]                                                 # long and thin, across several workgroups: the deepest parent chains
    ref = reference("chain", 0, 1.0, 1, 1, 0, mode)
    assert ref["sizes"].tolist() == [300]
    check(run(ctx, capi, chain, radius=1.0, dist_mode=mode), ref, "chain")
    ref = reference("chain", 0, 1.0, 3, 1, 0, mode)                           # the two ends are border points
    assert ref["sizes"].tolist() == [300] and ref["is_core"].sum() == 298
    check(run(ctx, capi, chain, radius=1.0, min_points=3, dist_mode=mode), ref, "chain, min_points 3")
    ref = reference("chain", 0, BELOW_ONE, 1, 1, 0, mode)
    assert ref["n_clusters"] == 300
    check(run(ctx, capi, chain, radius=BELOW_ONE, dist_mode=mode), ref, "chain below 1")


@pytest.mark.parametrize("mode", MODES)
def test_a_dense_ball_hooks_into_one_set(ctx, capi, mode):
    ref = reference("ball", 0, 0.25, 1, 1, 0, mode)
    assert ref["sizes"].tolist() == [4000]
    check(run(ctx, capi, clouds()["ball"], radius=0.25, dist_mode=mode), ref, "ball")


# ---- 3. blobs and noise
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("min_points", (1, 5, 12))
def test_blobs_and_noise(ctx, capi, min_points, mode):
    ref = reference("blobs", 0, BLOB_RADIUS, min_points, 1, 0, mode)
    if min_points == 5:                                                       # (the restatement alone: the input is not degenerate)
        border = (ref["is_core"] == 0) & (ref["labels"] >= 0)
        assert ref["n_clusters"] >= 3 and border.sum() > 0 and (ref["labels"] < 0).sum() > 0 and ref["sizes"].max() > 500
    check(run(ctx, capi, clouds()["blobs"], radius=BLOB_RADIUS, min_points=min_points, dist_mode=mode), ref, "blobs %d" % min_points)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", (257, 1024, 1025, 2049))
def test_workgroup_and_tile_edges(ctx, capi, n, mode):
    ref = reference("blobs", n, 0.6, 4, 1, 0, mode)
    assert ref["n_clusters"] >= 2
    check(run(ctx, capi, clouds()["blobs"][:n], radius=0.6, min_points=4, dist_mode=mode), ref, "n = %d" % n)


@pytest.mark.parametrize("mode", MODES)
def test_the_size_filter(ctx, capi, mode):
    cloud, which = filter_case()
    for fields in (dict(min_cluster_size=3), dict(max_cluster_size=4), dict(min_cluster_size=3, max_cluster_size=4), dict(min_cluster_size=6)):
        check(run(ctx, capi, cloud, radius=0.6, dist_mode=mode, **fields), R.dbscan(cloud, 0.6, 1, dist_mode=mode, **fields), str(fields))
    free = reference("blobs", 0, BLOB_RADIUS, 5, 1, 0, mode)
    for lo, hi in ((20, 0), (1, 800), (3, 1000)):
        ref = reference("blobs", 0, BLOB_RADIUS, 5, lo, hi, mode)
        assert 0 < ref["n_clusters"] < free["n_clusters"] and np.array_equal(ref["is_core"], free["is_core"])      # at least one cluster dissolved
        check(run(ctx, capi, clouds()["blobs"], radius=BLOB_RADIUS, min_points=5, min_cluster_size=lo, max_cluster_size=hi, dist_mode=mode), ref, "filter %d %d" % (lo, hi))


# ---- 4. the optional outputs
@pytest.mark.parametrize("mode", MODES)
def test_optional_outputs(ctx, capi, mode):
    cloud = clouds()["blobs"]
    ref = reference("blobs", 0, BLOB_RADIUS, 5, 1, 0, mode)
    n, nc = len(cloud), ref["n_clusters"]
    fields = dict(radius=BLOB_RADIUS, min_points=5, dist_mode=mode)
    for want in ((), ("sizes",), ("core",), ("grouped",)):
        check(run(ctx, capi, cloud, want=want, **fields), ref, "outputs %s" % (want,))
    # a cluster_cap below n_clusters: the first cluster_cap sizes, nothing behind them; n_grouped without grouped_index
    cap = 2
    assert nc > cap
    labels, sizes, n_clusters, n_grouped = np.empty(n, np.int32), np.full(nc, -7, np.int32), C.c_int(-7), C.c_int(-7)
    p = capi.cluster_params(**fields)
    rc = capi.cluster_dbscan_raw(ctx._h, cloud.ctypes.data, n, C.addressof(p), labels.ctypes.data, C.addressof(n_clusters), sizes.ctypes.data, cap, None, None,
                                 C.addressof(n_grouped))
    assert rc == capi.MI_OK and n_clusters.value == nc and n_grouped.value == len(ref["grouped"]) and np.array_equal(labels, ref["labels"])
    assert np.array_equal(sizes[:cap], ref["sizes"][:cap]) and (sizes[cap:] == -7).all()


def test_a_far_straggler(ctx, capi):
    ref = check_case(ctx, capi, clouds()["straggler"], "straggler", radius=0.6, min_points=3)           # a grid of mostly empty cells
    assert ref["n_clusters"] >= 2 and ref["labels"][-1] == -1
    assert check_case(ctx, capi, clouds()["straggler"], "straggler, min_points 1", radius=0.6)["labels"][-1] >= 0


# ---- 5. determinism and independence of the order, the grid and the curve
@pytest.mark.parametrize("mode", MODES)
def test_the_same_call_twice_gives_the_same_bytes(ctx, capi, mode):
    fields = dict(radius=BLOB_RADIUS, min_points=5, dist_mode=mode)
    a = run(ctx, capi, clouds()["blobs"], **fields)
    run(ctx, capi, clouds()["ball"], radius=0.25, dist_mode=mode)
    b = run(ctx, capi, clouds()["blobs"], **fields)
    assert a["n_clusters"] == b["n_clusters"] and all(a[k].tobytes() == b[k].tobytes() for k in ("labels", "sizes", "is_core", "grouped"))


@pytest.mark.parametrize("mode", MODES)
def test_a_permutation_gives_the_same_partition(ctx, capi, mode):
    cloud = clouds()["blobs"]
    perm = np.random.default_rng(7).permutation(len(cloud))
    fields = dict(radius=BLOB_RADIUS, min_points=1, dist_mode=mode)           # (no border points: their rule breaks exact ties by index)
    a, b = run(ctx, capi, cloud, **fields), run(ctx, capi, np.ascontiguousarray(cloud[perm]), **fields)
    back = np.empty(len(cloud), np.int32)
    back[perm] = b["labels"]                                                  # the permuted call's label of the caller's point i
    pairs = set(zip(a["labels"].tolist(), back.tolist()))
    assert a["n_clusters"] == b["n_clusters"] == len(pairs) == len({x for x, _ in pairs}) == len({y for _, y in pairs})
    fields["min_points"] = 5
    a, b = run(ctx, capi, cloud, **fields), run(ctx, capi, np.ascontiguousarray(cloud[perm]), **fields)
    core = np.empty(len(cloud), np.uint8)
    core[perm] = b["is_core"]
    back[perm] = b["labels"]
    assert np.array_equal(core, a["is_core"])
    on = a["is_core"] == 1                                                    # the core points' partition, and the noise set where no border rule is in play
    pairs = set(zip(a["labels"][on].tolist(), back[on].tolist()))
    assert len(pairs) == len({x for x, _ in pairs}) == len({y for _, y in pairs}) and np.array_equal(a["labels"] < 0, back < 0)


@pytest.mark.parametrize("variable,value", [("MISLAM_OUTLIER_RADIUS_CELL", "0.25"), ("MISLAM_OUTLIER_RADIUS_CELL", "4"), ("MISLAM_KNN_POINTS_PER_CELL", "0.25"),
                                            ("MISLAM_KNN_POINTS_PER_CELL", "1e9")])
def test_cell_regimes_give_the_same_answer(capi, monkeypatch, variable, value):
    monkeypatch.setenv(variable, value)
    with capi.Context(0) as c2:
        for mode in MODES:
            check(run(c2, capi, clouds()["blobs"][:2049], radius=0.6, min_points=4, dist_mode=mode), reference("blobs", 2049, 0.6, 4, 1, 0, mode), "%s=%s" % (variable, value))
            check(run(c2, capi, clouds()["chain"], radius=1.0, dist_mode=mode), reference("chain", 0, 1.0, 1, 1, 0, mode), "chain %s=%s" % (variable, value))


# ---- 6. refusals, times, buffers
def raw_call(ctx, capi, cloud, n, null=(), cap=None, **fields):
    """mi_cluster_dbscan with every output prefilled with a sentinel -> (error code, message, outputs untouched?)"""
    rows = max(n, 1)
    labels, sizes, core, grouped = np.full(rows, -7, np.int32), np.full(rows, -7, np.int32), np.full(rows, 7, np.uint8), np.full(rows, -7, np.int32)
    n_clusters, n_grouped = C.c_int(-7), C.c_int(-7)
    p = capi.cluster_params(**dict(dict(radius=0.5), **fields))
    arg = lambda name, value: None if name in null else value
    rc = capi.cluster_dbscan_raw(ctx._h, arg("cloud", cloud.ctypes.data), n, arg("params", C.addressof(p)), arg("labels", labels.ctypes.data),
                                 arg("n_clusters", C.addressof(n_clusters)), sizes.ctypes.data, rows if cap is None else cap, core.ctypes.data,
                                 grouped.ctypes.data, arg("n_grouped", C.addressof(n_grouped)))
    untouched = bool((labels == -7).all() and (sizes == -7).all() and (core == 7).all() and (grouped == -7).all() and n_clusters.value == -7 and n_grouped.value == -7)
    return rc, capi.lib().mi_last_error().decode(), untouched


def test_refusals_leave_the_outputs_untouched(ctx, capi):
    c = np.array(clouds()["blobs"][:1000])
    nan, inf = float("nan"), float("inf")
    bad_args = [dict(null=("cloud",)), dict(null=("params",)), dict(null=("labels",)), dict(null=("n_clusters",)), dict(null=("n_grouped",)), dict(n=0), dict(n=-1),
                dict(dist_mode=2), dict(dist_mode=-1), dict(min_points=0), dict(min_points=-3), dict(min_cluster_size=0), dict(max_cluster_size=-1),
                dict(min_cluster_size=5, max_cluster_size=4), dict(cap=0), dict(cap=-2)]
    bad_args += [dict(radius=v) for v in (nan, inf, 0.0, -1.0, 1e20)]                                   # (1e20: the square is not finite)
    for kw in bad_args:
        rc, msg, untouched = raw_call(ctx, capi, c, **dict(dict(n=1000), **kw))
        assert rc == capi.MI_ERR_INVALID_ARG and untouched and msg.startswith("mi_cluster_dbscan"), (kw, msg)
        named = ["cluster_cap" if k == "cap" else k for k in kw if k not in ("n", "null")] + ["cloud_xyz" if v == "cloud" else v for v in kw.get("null", ())]
        assert all(k in msg for k in named), (kw, msg)                  # the cause: the field's or the argument's name
    for value in (np.nan, np.inf, 1.5e18):                              # a bad point: its index -- the LOWEST one
        bc = c.copy()
        bc[917, 2] = value
        bc[333, 0] = value
        rc, msg, untouched = raw_call(ctx, capi, bc, 1000)
        assert rc == capi.MI_ERR_INVALID_ARG and untouched and msg.startswith("mi_cluster_dbscan") and "cloud_xyz point 333 " in msg, (value, msg)
    # and the context still works
    check(run(ctx, capi, clouds()["blobs"][:1025], radius=0.6, min_points=4), reference("blobs", 1025, 0.6, 4, 1, 0, K.DIST_CPU_ROUNDING), "after the refusals")


def test_stage_times(ctx, capi):
    run(ctx, capi, clouds()["blobs"], radius=BLOB_RADIUS, min_points=5)
    ms = ctx.cluster_dbscan_times()
    assert list(ms) == ["workspace", "upload", "grid", "count", "link", "resolve", "finish", "total"]
    assert all(v >= 0 for v in ms.values()) and ms["total"] > 0 and sum(v for k, v in ms.items() if k != "total") <= ms["total"] * (1 + 1e-9)


def test_a_destroyed_context_leaves_no_device_buffer_behind(capi, ctx):
    start = capi.selftest_live_buffers()
    with capi.Context(0) as c2:
        run(c2, capi, clouds()["blobs"][:1025], radius=0.6, min_points=4)
        assert capi.selftest_live_buffers() > start
    assert capi.selftest_live_buffers() == start
