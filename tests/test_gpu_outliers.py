"""GPU suite of mi_remove_outliers against the float64 restatement of tests/outlier_reference.py.  The O(n^2) part of the restatement,
the sorted keys of tests/knn_reference.py in self mode, is built once per cloud and arithmetic (lru_cache) and shared by every k.

The bounds (none of them taken from what the device gives):
  neighbours      equal to the restatement's
  mean_distance   |got - mu_ref| <= 6e-8 mu_ref: one fp32 rounding, 2^-24 = 5.96e-8; the fp64 sum of at most 32 roots adds about 4e-15.
                  Exactly 0 where mu_ref is 0.
  stats           mean, stddev and threshold each within 4 n 2^-53 (mean_ref + stddev_ref) of numpy's float64 on the restatement's mu,
                  the linear worst case of an n-term fp64 sum in any order; stddev exactly 0 when every mu_ref is equal
  keep            statistical: equal to mu_ref <= threshold_ref on every point with |mu_ref - threshold_ref| > 1e-9 threshold_ref (on the
                  three main clouds the restatement alone shows that this leaves no point out: the smallest margin is 7.6e-6);
                  radius: equal to the restatement's, exactly
  consistency     out_index = flatnonzero(keep), out_xyz = the bits of cloud[out_index], out_n = stats.kept = keep.sum(); asking for
                  fewer optional outputs gives the same bits in the rest"""
import functools

import numpy as np
import pytest

import knn_reference as K
import outlier_reference as R

pytestmark = pytest.mark.gpu

MODES = (K.DIST_CPU_ROUNDING, K.DIST_FMA)
CLOUDS = ("volume_outliers", "plane_outliers", "offset")
STATISTICAL, RADIUS = 0, 1
RATIOS = (0.0, 1.0, 2.0)


def frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def clouds():
    rng = np.random.default_rng(83)
    volume = np.concatenate([rng.uniform(-5, 5, (1900, 3)), rng.uniform(-50, 50, (100, 3))]).astype(np.float32)
    xy = rng.uniform(-5, 5, (1900, 2))
    plane = np.concatenate([xy, (0.3 * xy[:, 0] - 0.2 * xy[:, 1] + 0.02 * rng.normal(size=1900))[:, None]], axis=1)
    plane = np.concatenate([plane, rng.uniform(-5, 5, (100, 3))]).astype(np.float32)
    offset = (volume + np.array([100.0, -50.0, 25.0], np.float32)).astype(np.float32)
    return {"volume_outliers": frozen(volume), "plane_outliers": frozen(plane), "offset": frozen(offset)}


@functools.lru_cache(maxsize=None)
def cloud_keys(name, mode):
    return frozen(K.sorted_keys(None, clouds()[name], mode))


@functools.lru_cache(maxsize=None)
def ref_scores(name, k, mode):
    mu, count = R.scores(cloud_keys(name, mode), k)
    return frozen(mu), frozen(count)


@functools.lru_cache(maxsize=None)
def ref_radius_counts(name, radius, mode):
    return frozen(R.radius_counts(clouds()[name], radius, mode))


def lattice(side):
    g = np.arange(side, dtype=np.float32)
    z, y, x = np.meshgrid(g, g, g, indexing="ij")
    return np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1)       # index = x + side y + side^2 z


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype.itemsize == 4 else a


def stats_tuple(s):
    return (s.mean, s.stddev, s.threshold, s.kept)


def run(ctx, capi, cloud, want_keep=True, want_mean_distance=None, want_neighbours=True, want_stats=True, **fields):
    """One call -> dict of everything that was asked for (mean_distance by default whenever the method has one)."""
    p = capi.outlier_params(**fields)
    if want_mean_distance is None:
        want_mean_distance = p.method == STATISTICAL
    res = list(ctx.remove_outliers(cloud, p, want_keep=want_keep, want_mean_distance=want_mean_distance, want_neighbours=want_neighbours,
                                   want_stats=want_stats))
    out = {"xyz": res.pop(0), "index": res.pop(0)}
    for name, asked in (("keep", want_keep), ("mean_distance", want_mean_distance), ("neighbours", want_neighbours), ("stats", want_stats)):
        if asked:
            out[name] = res.pop(0)
    if want_stats:
        out["stats"] = stats_tuple(out["stats"])
    return out


def same_bits(a, b):
    """every output the two answers share, bit for bit"""
    for name in set(a) & set(b):
        if name == "stats":
            if np.array(a[name][:3], np.float64).tobytes() != np.array(b[name][:3], np.float64).tobytes() or a[name][3] != b[name][3]:
                return False
        elif not np.array_equal(bits(a[name]), bits(b[name])):
            return False
    return True


def check_consistency(cloud, got, what):
    keep = got["keep"]
    assert set(np.unique(keep).tolist()) <= {0, 1}, what
    assert np.array_equal(got["index"], np.flatnonzero(keep).astype(np.int32)), what
    assert got["xyz"].shape == (len(got["index"]), 3) and np.array_equal(bits(got["xyz"]), bits(cloud[got["index"]])), what
    assert len(got["index"]) == got["stats"][3] == int(keep.sum()), what


def check_statistical(cloud, got, mu, count, std_ratio, what, cap=True):
    """One statistical answer against the restatement's scores; returns the number of points the 1e-9 rule leaves out of the mask check."""
    n = len(cloud)
    mean, stddev, threshold = R.statistics(mu, std_ratio)
    assert np.array_equal(got["neighbours"], count), what
    md = got["mean_distance"].astype(np.float64)
    rel = np.abs(md - mu)[mu > 0] / mu[mu > 0]
    tol = 4 * n * 2.0 ** -53 * (mean + stddev)
    errs = [abs(got["stats"][0] - mean), abs(got["stats"][1] - stddev), abs(got["stats"][2] - threshold)]
    clear = np.abs(mu - threshold) > 1e-9 * threshold
    print("%s: mean_distance rel %.3e; |d mean| %.3e |d stddev| %.3e |d threshold| %.3e (bound %.3e); removed %d, left out of the mask check %d" % (
        what, rel.max(initial=0.0), errs[0], errs[1], errs[2], tol, n - got["stats"][3], (~clear).sum()))
    assert (np.abs(md - mu) <= 6e-8 * mu).all() and (md[mu == 0] == 0).all(), what
    assert max(errs) <= tol, what
    if (mu == mu[0]).all():
        assert got["stats"][1] == 0.0, what
    if cap:
        assert clear.all(), what                                      # (the restatement alone)
    assert np.array_equal(got["keep"][clear].astype(bool), (mu <= threshold)[clear]), what
    check_consistency(cloud, got, what)
    return int((~clear).sum())


def check_radius(cloud, got, count, min_neighbours, what):
    assert np.array_equal(got["neighbours"], count), what
    assert np.array_equal(got["keep"].astype(bool), count >= min_neighbours), what
    assert got["stats"][:3] == (0.0, 0.0, float(min_neighbours)), what
    check_consistency(cloud, got, what)


def fewer_outputs_agree(ctx, capi, cloud, full, **fields):
    """the same call with fewer optional outputs: the same bits in what is left (radius without neighbours: the early-exit kernel)"""
    assert same_bits(run(ctx, capi, cloud, want_neighbours=False, **fields), full), fields
    assert same_bits(run(ctx, capi, cloud, want_keep=False, want_mean_distance=False, want_neighbours=False, want_stats=False, **fields), full), fields
    assert same_bits(run(ctx, capi, cloud, want_keep=False, want_mean_distance=False, want_stats=False, **fields), full), fields


# ---- 1. statistical: every cloud, every list size and one past 16, both arithmetics, three ratios
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k", [1, 4, 8, 16, 17, 32])
@pytest.mark.parametrize("name", CLOUDS)
def test_statistical_filter(ctx, capi, name, k, mode):
    cloud = clouds()[name]
    mu, count = ref_scores(name, k, mode)
    for ratio in RATIOS:
        fields = dict(method=STATISTICAL, k=k, dist_mode=mode, std_ratio=ratio)
        got = run(ctx, capi, cloud, **fields)
        check_statistical(cloud, got, mu, count, ratio, "%s k %d mode %d ratio %g" % (name, k, mode, ratio))
        if k != 17:
            assert 69 <= len(cloud) - got["stats"][3] <= 483          # (what the restatement alone removes at these k and ratios)
        if ratio == 1.0:
            fewer_outputs_agree(ctx, capi, cloud, got, **fields)


# ---- 2. radius: every cloud, three radii, four thresholds, both arithmetics
KEPT = {("volume_outliers", 4): (18, 1673, 1900), ("volume_outliers", 40): (0, 0, 1428),
        ("plane_outliers", 4): (1905, 1917, 1958), ("plane_outliers", 40): (0, 1633, 1933)}     # at radius 0.5 / 1 / 2


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("radius", [0.5, 1.0, 2.0])
@pytest.mark.parametrize("name", CLOUDS)
def test_radius_filter(ctx, capi, name, radius, mode):
    cloud = clouds()[name]
    count = ref_radius_counts(name, radius, mode)
    for min_nb in (1, 4, 40, 5000):
        if (name, min_nb) in KEPT and mode == K.DIST_CPU_ROUNDING:
            assert int((count >= min_nb).sum()) == KEPT[(name, min_nb)][(0.5, 1.0, 2.0).index(radius)]
        fields = dict(method=RADIUS, radius=radius, min_neighbours=min_nb, dist_mode=mode)
        got = run(ctx, capi, cloud, **fields)
        check_radius(cloud, got, count, min_nb, "%s radius %g min %d mode %d" % (name, radius, min_nb, mode))
        if min_nb == 5000:
            assert got["stats"][3] == 0 and len(got["index"]) == 0 and not got["keep"].any()
        fewer_outputs_agree(ctx, capi, cloud, got, **fields)


# ---- 3. ties at the radius
@pytest.mark.parametrize("mode", MODES)
def test_ties_at_the_radius(ctx, capi, mode):
    L = lattice(3)
    on_boundary = ((L == 0) | (L == 2)).sum(axis=1)
    got = run(ctx, capi, L, method=RADIUS, radius=1.0, min_neighbours=4, dist_mode=mode)
    assert np.array_equal(got["neighbours"], 6 - on_boundary) and np.array_equal(got["keep"].astype(bool), on_boundary < 3)
    check_consistency(L, got, "lattice radius 1")
    below = float(np.nextafter(np.float32(1), np.float32(0)))
    assert np.float32(0.99999994) == np.float32(below) and below < 1          # 0.99999994 names the float below 1
    got = run(ctx, capi, L, method=RADIUS, radius=below, min_neighbours=1, dist_mode=mode)
    assert (got["neighbours"] == 0).all() and got["stats"][3] == 0
    # every point stored twice, a radius whose square underflows to +0: the twin is the one neighbour
    twins = np.concatenate([clouds()["volume_outliers"][:500], clouds()["volume_outliers"][:500]])
    assert np.float32(1e-30) * np.float32(1e-30) == 0
    got = run(ctx, capi, twins, method=RADIUS, radius=1e-30, min_neighbours=1, dist_mode=mode)
    assert (got["neighbours"] == 1).all() and got["keep"].all() and got["stats"][3] == 1000
    check_consistency(twins, got, "twins")
    fewer_outputs_agree(ctx, capi, twins, got, method=RADIUS, radius=1e-30, min_neighbours=1, dist_mode=mode)
    got = run(ctx, capi, twins, method=RADIUS, radius=1e-30, min_neighbours=2, dist_mode=mode)
    assert (got["neighbours"] == 1).all() and got["stats"][3] == 0 and len(got["xyz"]) == 0


# ---- 4. the smallest shapes: the one-wave workgroup's edge, every list size at its edge and one past it; the compaction's tile and the
# statistics' block, one below, at, one above and one above twice that
def small_case(ctx, capi, n, ks):
    rng = np.random.default_rng(1000 + n)
    cloud = rng.uniform(-5, 5, (n, 3)).astype(np.float32)
    left_out = 0
    for mode in MODES:
        keys = K.sorted_keys(None, cloud, mode)
        for k in ks:
            mu, count = R.scores(keys, k)
            assert (count == min(k, n - 1)).all()
            for ratio in (0.0, 1.0):
                got = run(ctx, capi, cloud, method=STATISTICAL, k=k, dist_mode=mode, std_ratio=ratio)
                left_out += check_statistical(cloud, got, mu, count, ratio, "n %d k %d mode %d ratio %g" % (n, k, mode, ratio), cap=False)
                if n == 1:
                    assert got["keep"].tolist() == [1] and got["stats"] == (0.0, 0.0, 0.0, 1)
        count = R.radius_counts(cloud, 3.0, mode)
        for min_nb in (1, 3):
            fields = dict(method=RADIUS, radius=3.0, min_neighbours=min_nb, dist_mode=mode)
            got = run(ctx, capi, cloud, **fields)
            check_radius(cloud, got, count, min_nb, "n %d radius 3 min %d mode %d" % (n, min_nb, mode))
            fewer_outputs_agree(ctx, capi, cloud, got, **fields)
            if n == 1:
                assert got["keep"].tolist() == [0] and got["stats"][3] == 0
    print("n %d: %d points left out of the mask checks" % (n, left_out))


@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 127, 129])
def test_smallest_shapes(ctx, capi, n):
    small_case(ctx, capi, n, [1, 8, 9, 16, 17, 32])


@pytest.mark.parametrize("n", [255, 256, 257, 513, 1023, 1024, 1025, 2049])
def test_sizes_around_the_statistics_block_and_the_compaction_tile(ctx, capi, n):
    small_case(ctx, capi, n, [8])


# ---- 5. compaction across many tiles, with an analytic answer
@pytest.mark.parametrize("mode", MODES)
def test_lattice_41_interior_is_what_stays(ctx, capi, mode):
    side = 41
    L = lattice(side)
    on_boundary = ((L == 0) | (L == side - 1)).sum(axis=1)
    interior = np.flatnonzero(on_boundary == 0).astype(np.int32)
    assert len(interior) == 39 ** 3
    got = run(ctx, capi, L, method=RADIUS, radius=1.0, min_neighbours=6, dist_mode=mode)
    assert np.array_equal(got["neighbours"], 6 - on_boundary)
    assert np.array_equal(got["index"], interior) and np.array_equal(bits(got["xyz"]), bits(L[interior]))
    check_consistency(L, got, "lattice 41 radius")
    fewer_outputs_agree(ctx, capi, L, got, method=RADIUS, radius=1.0, min_neighbours=6, dist_mode=mode)
    # statistical, k = 6: an interior point's six neighbours are at 1; on a face five are and the sixth at sqrt 2, on an edge four and
    # two, at a corner three and three -- so mu = 1 inside, above the mean outside, and at ratio 0 the interior is what stays
    got = run(ctx, capi, L, method=STATISTICAL, k=6, std_ratio=0.0, dist_mode=mode)
    s2 = np.sqrt(2.0)
    mu_class = np.array([1.0, (5 + s2) / 6, ((4 + s2) + s2) / 6, (((3 + s2) + s2) + s2) / 6])
    members = np.array([39 ** 3, 6 * 39 ** 2, 12 * 39, 8], np.float64)
    assert np.array_equal(np.bincount(on_boundary, minlength=4), members.astype(np.int64))
    n = side ** 3
    mean = float((members * mu_class).sum() / n)
    stddev = float(np.sqrt((members * (mu_class - mean) ** 2).sum() / n))
    tol = 4 * n * 2.0 ** -53 * (mean + stddev)
    print("lattice 41 mode %d: |d mean| %.3e |d stddev| %.3e (bound %.3e)" % (mode, abs(got["stats"][0] - mean), abs(got["stats"][1] - stddev), tol))
    assert abs(got["stats"][0] - mean) <= tol and abs(got["stats"][1] - stddev) <= tol and abs(got["stats"][2] - mean) <= tol
    assert (got["neighbours"] == 6).all()
    assert (np.abs(got["mean_distance"].astype(np.float64) - mu_class[on_boundary]) <= 6e-8 * mu_class[on_boundary]).all()
    assert np.array_equal(got["index"], interior) and np.array_equal(bits(got["xyz"]), bits(L[interior]))
    check_consistency(L, got, "lattice 41 statistical")


# ---- 6. awkward clouds (those of tests/test_gpu_normals.py, built here)
def awkward_cloud(kind):
    rng = np.random.default_rng(41)
    m = 1000
    if kind == "identical":
        return np.tile(np.array([[1.5, -2.25, 3.0]], np.float32), (m, 1))
    if kind == "collinear":
        t = rng.uniform(-5, 5, m).astype(np.float32)
        return np.stack([t, np.float32(2) * t, np.float32(-1) * t], axis=1).astype(np.float32)
    if kind == "coplanar":
        c = rng.uniform(-5, 5, (m, 3)).astype(np.float32)
        c[:, 2] = 0.75
        return c
    if kind == "two_clusters":
        c = rng.normal(scale=0.05, size=(m, 3))
        c[m // 2:] += 1e3
        return c.astype(np.float32)
    if kind == "outlier":
        c = rng.normal(scale=0.5, size=(m, 3))
        c[m - 1] = 1e6
        return c.astype(np.float32)
    assert kind == "offset"                      # fp32 spacing at 1e5 is 2^-7: many exact ties
    return (1e5 + rng.uniform(0, 1, (m, 3))).astype(np.float32)


@pytest.mark.parametrize("kind", ["identical", "collinear", "coplanar", "two_clusters", "outlier", "offset"])
def test_awkward_clouds(ctx, capi, kind):
    cloud = awkward_cloud(kind)
    for mode in MODES:
        mu, count = R.scores(K.sorted_keys(None, cloud, mode), 8)
        for ratio in RATIOS:
            got = run(ctx, capi, cloud, method=STATISTICAL, k=8, dist_mode=mode, std_ratio=ratio)
            left_out = check_statistical(cloud, got, mu, count, ratio, "%s mode %d ratio %g" % (kind, mode, ratio), cap=False)
            print("%s mode %d ratio %g: %d points left out of the mask check" % (kind, mode, ratio, left_out))
            if kind == "identical":
                assert got["keep"].all() and got["stats"] == (0.0, 0.0, 0.0, 1000)
            if kind == "outlier" and ratio == 2.0:
                assert got["keep"][999] == 0 and got["keep"].sum() >= 900
        rcount = R.radius_counts(cloud, 1.0, mode)
        got = run(ctx, capi, cloud, method=RADIUS, radius=1.0, min_neighbours=1, dist_mode=mode)
        check_radius(cloud, got, rcount, 1, "%s radius 1 mode %d" % (kind, mode))
        fewer_outputs_agree(ctx, capi, cloud, got, method=RADIUS, radius=1.0, min_neighbours=1, dist_mode=mode)
        if kind == "outlier":
            assert got["keep"][999] == 0 and got["keep"].sum() >= 900
        if kind == "identical":
            assert (got["neighbours"] == 999).all()


# ---- 7. every cell regime gives the default's bits
def regime_calls(c, capi, cloud):
    out = []
    for mode in MODES:
        out.append(run(c, capi, cloud, method=STATISTICAL, k=16, dist_mode=mode, std_ratio=1.0))
        out.append(run(c, capi, cloud, method=RADIUS, radius=1.0, min_neighbours=4, dist_mode=mode))
        out.append(run(c, capi, cloud, method=RADIUS, radius=1.0, min_neighbours=4, dist_mode=mode, want_neighbours=False))
    return out


@pytest.mark.parametrize("variable,value", [("MISLAM_KNN_POINTS_PER_CELL", "0.25"), ("MISLAM_KNN_POINTS_PER_CELL", "8"), ("MISLAM_KNN_POINTS_PER_CELL", "1e9"),
                                            ("MISLAM_OUTLIER_RADIUS_CELL", "0.25"), ("MISLAM_OUTLIER_RADIUS_CELL", "4")])
def test_cell_regimes_give_the_same_bits(ctx, capi, monkeypatch, variable, value):
    cloud = clouds()["plane_outliers"]           # (2000 points in a box of 10: a cell of 0.25, 1 and 4 radii are three different grids)
    want = regime_calls(ctx, capi, cloud)
    monkeypatch.setenv(variable, value)
    with capi.Context(0) as c2:
        for w, g in zip(want, regime_calls(c2, capi, cloud)):
            assert same_bits(g, w) and set(g) == set(w), (variable, value)


# ---- 8. context hygiene
def test_a_loaded_icp_problem_survives_and_calls_do_not_leak_into_each_other(ctx, capi, golden):
    z = golden.npz("synth2k_clouds.npz")
    params = capi.icp_params(max_iterations=8)
    ctx.icp_load(z["before"], z["after"], params)
    ctx.icp_run(8)
    R0, t0, it0, err0, why0 = ctx.icp_result()
    ctx.icp_load(z["before"], z["after"], params)
    cloud = clouds()["offset"]
    knn_first = ctx.knn_search(None, cloud, 8, K.DIST_FMA, want_count=True)
    normals_first = ctx.estimate_normals(cloud, 8, None, K.DIST_FMA, want_curvature=True, want_count=True)
    first = run(ctx, capi, cloud, method=STATISTICAL, k=8, dist_mode=K.DIST_FMA)
    first_radius = run(ctx, capi, cloud, method=RADIUS, radius=1.0, min_neighbours=4, dist_mode=K.DIST_FMA)
    ctx.icp_run(8)
    R1, t1, it1, err1, why1 = ctx.icp_result()
    assert it0 > 0 and (it1, why1) == (it0, why0)
    assert np.array_equal(bits(R1), bits(R0)) and np.array_equal(bits(t1), bits(t0))
    assert np.float32(err1).tobytes() == np.float32(err0).tobytes()
    # calls of other sizes and methods in between leave nothing behind
    run(ctx, capi, clouds()["volume_outliers"][:65], method=STATISTICAL, k=32, std_ratio=0.5)
    run(ctx, capi, z["after"], method=RADIUS, radius=0.25, min_neighbours=2, want_neighbours=False)
    assert same_bits(run(ctx, capi, cloud, method=STATISTICAL, k=8, dist_mode=K.DIST_FMA), first)
    assert same_bits(run(ctx, capi, cloud, method=RADIUS, radius=1.0, min_neighbours=4, dist_mode=K.DIST_FMA), first_radius)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(ctx.knn_search(None, cloud, 8, K.DIST_FMA, want_count=True), knn_first))
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(ctx.estimate_normals(cloud, 8, None, K.DIST_FMA, want_curvature=True, want_count=True), normals_first))


# ---- 9. refusals: nothing is written
def raw_call(ctx, capi, cloud, n, null_params=False, null_out_n=False, **fields):
    """mi_remove_outliers with every output prefilled with a sentinel -> (error code, message, outputs untouched?)"""
    import ctypes as C
    rows = max(n, 1)
    xyz, index, keep = np.full(3 * rows, -7.5, np.float32), np.full(rows, -7, np.int32), np.full(rows, 7, np.uint8)
    mean_distance, neighbours = np.full(rows, -7.5, np.float32), np.full(rows, -7, np.int32)
    out_n, stats = C.c_int(-7), capi.OutlierStats(-7.5, -7.5, -7.5, -7)
    p = capi.outlier_params(**fields)
    rc = capi.remove_outliers_raw(ctx._h, None if cloud is None else cloud.ctypes.data, n, None if null_params else C.addressof(p), xyz.ctypes.data,
                                  index.ctypes.data, None if null_out_n else C.addressof(out_n), keep.ctypes.data, mean_distance.ctypes.data,
                                  neighbours.ctypes.data, C.addressof(stats))
    untouched = bool((xyz == -7.5).all() and (index == -7).all() and (keep == 7).all() and (mean_distance == -7.5).all() and (neighbours == -7).all()
                     and out_n.value == -7 and stats_tuple(stats) == (-7.5, -7.5, -7.5, -7))
    return rc, capi.lib().mi_last_error().decode(), untouched


def test_refusals_leave_the_outputs_untouched(ctx, capi):
    c = np.array(clouds()["volume_outliers"][:1000])
    nan, inf = float("nan"), float("inf")
    rad = dict(method=RADIUS, radius=1.0, min_neighbours=2)
    bad_args = [
        dict(cloud=None, n=1000), dict(cloud=c, n=1000, null_params=True), dict(cloud=c, n=1000, null_out_n=True),
        dict(cloud=c, n=0), dict(cloud=c, n=-1),
        dict(cloud=c, n=1000, method=2), dict(cloud=c, n=1000, method=-1), dict(cloud=c, n=1000, dist_mode=2), dict(cloud=c, n=1000, dist_mode=-1),
        dict(cloud=c, n=1000, k=0), dict(cloud=c, n=1000, k=-1), dict(cloud=c, n=1000, k=33),
        dict(cloud=c, n=1000, std_ratio=nan), dict(cloud=c, n=1000, std_ratio=inf), dict(cloud=c, n=1000, std_ratio=-0.5),
        dict(cloud=c, n=1000, **dict(rad, radius=nan)), dict(cloud=c, n=1000, **dict(rad, radius=inf)), dict(cloud=c, n=1000, **dict(rad, radius=0.0)),
        dict(cloud=c, n=1000, **dict(rad, radius=-1.0)), dict(cloud=c, n=1000, **dict(rad, radius=1e20)),
        dict(cloud=c, n=1000, **dict(rad, min_neighbours=0)), dict(cloud=c, n=1000, **dict(rad, min_neighbours=-3)),
    ]
    for kw in bad_args:
        rc, msg, untouched = raw_call(ctx, capi, **kw)
        assert rc == capi.MI_ERR_INVALID_ARG and untouched and msg.startswith("mi_remove_outliers"), (kw, msg)
    # a bad point: its index -- the LOWEST one, in mi_knn_search's wording
    for value in (np.nan, np.inf, -np.inf, 1.5e18, -1.5e18):
        bc = c.copy()
        bc[917, 2] = value
        bc[333, 0] = value
        for fields in (dict(), rad):
            rc, msg, untouched = raw_call(ctx, capi, bc, 1000, **fields)
            assert rc == capi.MI_ERR_INVALID_ARG and untouched and msg.startswith("mi_remove_outliers") and "cloud_xyz point 333 " in msg, (value, msg)
            rc2 = capi.knn_search_raw(ctx._h, None, 1000, bc.ctypes.data, 1000, 8, 0, float("inf"), np.empty(8000, np.int32).ctypes.data, None, None)
            assert rc2 == capi.MI_ERR_INVALID_ARG and capi.lib().mi_last_error().decode() == msg.replace("mi_remove_outliers", "mi_knn_search")
    with pytest.raises(capi.MiSlamError) as e:
        bc = c.copy()
        bc[5, 0] = np.nan
        ctx.remove_outliers(bc, capi.outlier_params())
    assert "cloud_xyz point 5 " in str(e.value)
    # the largest coordinates the call accepts: everything stays finite
    big = np.array([[1e18, -1e18, 1e18], [-1e18, 1e18, -1e18], [0, 0, 0], [1e18, 1e18, 0]], np.float32)
    got = run(ctx, capi, big, method=STATISTICAL, k=3, dist_mode=K.DIST_FMA)
    assert (got["neighbours"] == 3).all() and np.isfinite(got["mean_distance"]).all() and np.isfinite(got["stats"][:3]).all()
    check_consistency(big, got, "corners")
    got = run(ctx, capi, big, method=RADIUS, radius=1e18, min_neighbours=1, dist_mode=K.DIST_FMA)
    check_radius(big, got, R.radius_counts(big, 1e18, K.DIST_FMA), 1, "corners radius")
    # and the context still works
    mu, count = ref_scores("volume_outliers", 8, K.DIST_CPU_ROUNDING)
    check_statistical(clouds()["volume_outliers"], run(ctx, capi, clouds()["volume_outliers"], method=STATISTICAL, k=8, std_ratio=2.0), mu, count, 2.0, "after the refusals")
