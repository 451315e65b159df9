"""GPU suite of mi_fpfh_features against the float64 restatement of tests/fpfh_reference.py.  The O(n^2) part of the restatement, the
sorted keys of tests/knn_reference.py in self mode, is built once per cloud and arithmetic (lru_cache) and shared by every k.

The bounds (fpfh_reference.check; none of them taken from what the device gives):
  count, counts   equal; every block of 11 counts sums to count
  fpfh            |got - ref| <= 2^-23 |ref|: one fp32 rounding, 2^-24, doubled (the fp64 chain of at most 32 x 2 operations adds about
                  1e-14); exactly 0 where ref is exactly 0 -- a zero arises only from zero counts, which are exact
  fragile points  (a pair of theirs or of a neighbour's within 1e-9 bin widths of a bin edge, or at a tie of the frame's choice, or with a
                  frame that is nearly undefined: fpfh_reference.py) keep the sums only: blocks of counts sum to count, blocks of fpfh to
                  200 within 2^-23 x 200.  A test may leave out at most 0.1 % of its points this way."""
import functools

import numpy as np
import pytest

import fpfh_reference as F
import knn_reference as K

pytestmark = pytest.mark.gpu

MODES = (K.DIST_CPU_ROUNDING, K.DIST_FMA)
CLOUDS = ("sphere", "sphere_offset", "volume", "plane_noise")


def frozen(a):
    a.setflags(write=False)
    return a


def unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def shell(rng, n):
    """(points, normals) float64: a noisy unit sphere; the normals are the directions plus noise of 0.05, of unit length"""
    d = unit(rng.normal(size=(n, 3)))
    return d * (1 + 0.01 * rng.normal(size=n))[:, None], unit(d + 0.05 * rng.normal(size=(n, 3)))


@functools.lru_cache(maxsize=None)
def clouds():
    """name -> (cloud, normals), float32 [2000, 3] each"""
    rng = np.random.default_rng(71)
    n = 2000
    out = {"sphere": shell(rng, n)}
    p, nr = shell(rng, n)
    out["sphere_offset"] = (p + np.array([100.0, -50.0, 25.0]), nr)
    out["volume"] = (rng.uniform(-5, 5, (n, 3)), unit(rng.normal(size=(n, 3))))
    xy = rng.uniform(-5, 5, (n, 2))
    plane = np.concatenate([xy, (0.3 * xy[:, 0] - 0.2 * xy[:, 1] + 0.02 * rng.normal(size=n))[:, None]], axis=1)
    out["plane_noise"] = (plane, unit(unit(np.array([[-0.3, 0.2, 1.0]])) + 0.05 * rng.normal(size=(n, 3))))
    return {name: (frozen(np.ascontiguousarray(c, np.float32)), frozen(np.ascontiguousarray(nr, np.float32))) for name, (c, nr) in out.items()}


@functools.lru_cache(maxsize=None)
def cloud_keys(name, mode):
    return frozen(K.sorted_keys(None, clouds()[name][0], mode))


@functools.lru_cache(maxsize=None)
def reference(name, k, mode):
    idx, d2, _ = K.unpack(cloud_keys(name, mode), k)
    return F.from_neighbours(*clouds()[name], idx, d2)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype.itemsize == 4 else a


def same_bits(got, want):
    return all(np.array_equal(bits(g), bits(w)) for g, w in zip(got, want))


def call(ctx, cloud, normals, k, mode=K.DIST_CPU_ROUNDING, max_d2=np.inf):
    return ctx.fpfh_features(cloud, normals, k, mode, max_d2, want_counts=True, want_count=True)


# ---- 1. every cloud, every list size, both arithmetics
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k", [4, 8, 16, 32])
@pytest.mark.parametrize("name", CLOUDS)
def test_counts_count_and_fpfh(ctx, name, k, mode):
    cloud, normals = clouds()[name]
    got = call(ctx, cloud, normals, k, mode)
    F.check(reference(name, k, mode), got, "%s k %d mode %d" % (name, k, mode))
    # the descriptor alone is the same answer
    assert np.array_equal(bits(ctx.fpfh_features(cloud, normals, k, mode)), bits(got[0]))


# ---- 2. the distance limit
@pytest.mark.parametrize("mode", MODES)
def test_distance_limit(ctx, mode):
    cloud, normals = clouds()["sphere"]
    k = 4
    limit = float(np.quantile(K.unpack(cloud_keys("sphere", mode), k)[1][:, k - 1], 2.0 / 3.0))     # a third of the points are cut short
    idx, d2, count = K.knn(None, cloud, k, mode, limit)
    assert 0.25 * len(cloud) < (count < k).sum() < 0.4 * len(cloud) and 0 < (count == 0).sum() < 50
    got = call(ctx, cloud, normals, k, mode, limit)
    F.check(F.from_neighbours(cloud, normals, idx, d2), got, "sphere limit %g mode %d" % (limit, mode))
    assert (got[0][count == 0] == 0).all() and (got[1][count == 0] == 0).all()
    assert np.array_equal(got[2], ctx.knn_search(None, cloud, k, mode, limit, want_d2=False, want_count=True)[1])


# ---- 3. small and degenerate shapes
def small_case(kind):
    """(cloud, normals, k)"""
    rng = np.random.default_rng(83)
    rand = lambda n: (rng.uniform(-1, 1, (n, 3)).astype(np.float32), unit(rng.normal(size=(n, 3))).astype(np.float32))
    if kind == "one_point":
        return rand(1) + (4,)
    if kind == "two_points":
        return rand(2) + (4,)
    if kind == "five_points_k8":
        return rand(5) + (8,)
    if kind == "identical":
        return np.tile(np.array([[1.5, -2.25, 3.0]], np.float32), (300, 1)), rand(300)[1], 8
    if kind == "lattice":
        g = np.arange(5, dtype=np.float32)
        return np.stack([np.repeat(g, 5), np.tile(g, 5), np.zeros(25, np.float32)], axis=1), np.tile(np.array([[0, 0, 1]], np.float32), (25, 1)), 8
    if kind == "duplicates":
        c, nr = rand(1000)
        c[900:] = c[:100]
        return c, nr, 8
    if kind == "zero_normals":
        return rand(500)[0], np.zeros((500, 3), np.float32), 8
    if kind == "long_normals":
        c, nr = rand(500)
        return c, np.float32(3) * nr, 8
    assert kind == "outlier"
    c, nr = rand(500)
    c[499] = 1e6
    return c, nr, 8


@pytest.mark.parametrize("kind", ["one_point", "two_points", "five_points_k8", "identical", "lattice", "duplicates", "zero_normals", "long_normals", "outlier"])
def test_small_and_degenerate_shapes(ctx, kind):
    cloud, normals, k = small_case(kind)
    n = len(cloud)
    for mode in MODES:
        ref = F.fpfh(cloud, normals, k, mode)
        got = call(ctx, cloud, normals, k, mode)
        assert all(np.isfinite(g).all() for g in got)
        F.check(ref, got, "%s mode %d" % (kind, mode), max_fragile_share=0.0)
        fpfh, counts, count = got
        if kind == "one_point":
            assert (fpfh == 0).all() and (counts == 0).all() and (count == 0).all()
        if kind == "five_points_k8":
            assert (count == 4).all()
        if kind in ("identical", "lattice", "zero_normals"):                  # every pair is degenerate: len 0, d across equal normals, u = 0
            want = np.zeros((n, 33), np.int64)
            want[:, [5, 16, 27]] = k
            assert np.array_equal(counts, want)
            assert np.array_equal(fpfh, np.where(want > 0, np.float32(100.0 if kind == "identical" else 200.0), np.float32(0)))


# ---- 4. beyond one grid row and 16-bit indices; the partial last workgroup; the second pass's gather across workgroups
def test_seventy_thousand_points(ctx):
    rng = np.random.default_rng(97)
    n, k = 70001, 16
    p, nr = shell(rng, n)
    cloud, normals = p.astype(np.float32), nr.astype(np.float32)
    idx, d2, count = ctx.knn_search(None, cloud, k, want_count=True)            # (tested on its own: tests/test_gpu_knn.py)
    assert (count == k).all()
    F.check(F.from_neighbours(cloud, normals, idx, d2), call(ctx, cloud, normals, k), "sphere of %d" % n)


# ---- 5. determinism and context hygiene
def test_the_same_bits_whatever_ran_before(ctx, capi, golden):
    cloud, normals = clouds()["sphere_offset"]
    first = call(ctx, cloud, normals, 16, K.DIST_FMA)
    assert same_bits(call(ctx, cloud, normals, 16, K.DIST_FMA), first)
    z = golden.npz("synth2k_clouds.npz")
    params = capi.icp_params(max_iterations=8)
    ctx.icp_load(z["before"], z["after"], params)
    ctx.icp_run(8)
    R0, t0, it0, err0, why0 = ctx.icp_result()
    ctx.icp_load(z["before"], z["after"], params)
    ctx.knn_search(None, clouds()["volume"][0], 8)
    ctx.estimate_normals(clouds()["volume"][0][:777], 32)
    ctx.remove_outliers(clouds()["plane_noise"][0], capi.outlier_params())
    call(ctx, *clouds()["volume"], 5, K.DIST_CPU_ROUNDING, 1.0)
    assert same_bits(call(ctx, cloud, normals, 16, K.DIST_FMA), first)
    ctx.icp_run(8)
    R1, t1, it1, err1, why1 = ctx.icp_result()
    assert it0 > 0 and (it1, why1) == (it0, why0)
    assert np.array_equal(bits(R1), bits(R0)) and np.array_equal(bits(t1), bits(t0))
    assert np.float32(err1).tobytes() == np.float32(err0).tobytes()


# ---- 6. refusals: nothing is written
def raw_call(ctx, capi, cloud, normals, n, k, mode=0, max_d2=np.inf, null_fpfh=False):
    """mi_fpfh_features with every output prefilled with a sentinel -> (error code, message, outputs untouched?)"""
    rows = max(n, 1)
    fpfh, counts, count = np.full(33 * rows, -7.5, np.float32), np.full(33 * rows, 7, np.uint8), np.full(rows, -7, np.int32)
    rc = capi.fpfh_features_raw(ctx._h, None if cloud is None else cloud.ctypes.data, None if normals is None else normals.ctypes.data, n, k, mode, float(max_d2),
                                None if null_fpfh else fpfh.ctypes.data, counts.ctypes.data, count.ctypes.data)
    return rc, capi.lib().mi_last_error().decode(), bool((fpfh == -7.5).all() and (counts == 7).all() and (count == -7).all())


def test_refusals_leave_the_outputs_untouched(ctx, capi):
    c, nr = (np.array(a[:1000]) for a in clouds()["volume"])
    bad_args = [
        dict(n=1000, k=0), dict(n=1000, k=33), dict(n=1000, k=-1),
        dict(n=1000, k=8, mode=2), dict(n=1000, k=8, mode=-1),
        dict(n=1000, k=8, max_d2=float("nan")), dict(n=1000, k=8, max_d2=-1.0), dict(n=1000, k=8, max_d2=float("-inf")),
        dict(n=1000, k=8, cloud=None), dict(n=1000, k=8, normals=None), dict(n=1000, k=8, null_fpfh=True),
        dict(n=0, k=8), dict(n=-1, k=8),
    ]
    for kw in bad_args:
        rc, msg, untouched = raw_call(ctx, capi, **dict(dict(cloud=c, normals=nr), **kw))
        assert rc == capi.MI_ERR_INVALID_ARG and untouched and msg.startswith("mi_fpfh_features: "), (kw, msg)
    # a bad value: which array, and its index -- the LOWEST one; the cloud is looked at first
    for value in (np.nan, np.inf, -np.inf, 1.5e18, -1.5e18):
        bc, bn = c.copy(), nr.copy()
        bc[917, 2] = value
        bc[333, 0] = value
        rc, msg, untouched = raw_call(ctx, capi, bc, nr, 1000, 8)
        assert rc == capi.MI_ERR_INVALID_ARG and untouched and msg.startswith("mi_fpfh_features: ") and "cloud_xyz point 333 " in msg, (value, msg)
        bn[640, 1] = value
        bn[212, 2] = value
        rc, msg, untouched = raw_call(ctx, capi, c, bn, 1000, 8)
        assert rc == capi.MI_ERR_INVALID_ARG and untouched and msg.startswith("mi_fpfh_features: ") and "normals_xyz normal 212 " in msg, (value, msg)
        rc, msg, untouched = raw_call(ctx, capi, bc, bn, 1000, 8)
        assert rc == capi.MI_ERR_INVALID_ARG and untouched and "cloud_xyz point 333 " in msg, (value, msg)
    with pytest.raises(capi.MiSlamError) as e:
        bn = nr.copy()
        bn[5, 0] = np.nan
        ctx.fpfh_features(c, bn, 8)
    assert "normals_xyz normal 5 " in str(e.value)
    with pytest.raises(ValueError):
        ctx.fpfh_features(c, nr[:999], 8)
    # and the context still works
    F.check(reference("volume", 8, 0), call(ctx, *clouds()["volume"], 8), "after the refusals")


# ---- 7. the descriptor itself: a rigid motion of the cloud and its normals leaves the counts alone
def moved_sphere():
    """the sphere cloud and its normals turned by 0.7 rad about (1, 2, 3) and shifted by (0.5, -1.25, 2), rounded to fp32"""
    cloud, normals = clouds()["sphere"]
    axis = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    R = np.eye(3) + np.sin(0.7) * Kx + (1 - np.cos(0.7)) * (Kx @ Kx)
    return (cloud.astype(np.float64) @ R.T + np.array([0.5, -1.25, 2.0])).astype(np.float32), (normals.astype(np.float64) @ R.T).astype(np.float32)


def comparable(ref_a, ref_b, idx_a, idx_b):
    """points whose neighbour lists are the same sets in both clouds and that are fragile in neither"""
    return (np.sort(idx_a, axis=1) == np.sort(idx_b, axis=1)).all(axis=1) & ~ref_a[3] & ~ref_b[3]


def test_rigid_motion_leaves_the_counts_alone(ctx):
    """Rounding the moved cloud to fp32 moves every feature by about 1e-7, so a pair within that of a bin edge may change its bin without
    being fragile in either cloud.  The restatement alone, on the CPU, compares 2000 of the 2000 points at k = 8 for this motion (every
    neighbour set survives the rounding, no point is fragile in either cloud) and finds the counts of all of them equal."""
    cloud, normals = clouds()["sphere"]
    moved, moved_normals = moved_sphere()
    k = 8
    idx_a, d2_a, _ = K.unpack(cloud_keys("sphere", 0), k)
    idx_b, d2_b, _ = K.knn(None, moved, k)
    ref_a, ref_b = reference("sphere", k, 0), F.from_neighbours(moved, moved_normals, idx_b, d2_b)
    both = comparable(ref_a, ref_b, idx_a, idx_b)
    got_a, got_b = call(ctx, cloud, normals, k), call(ctx, moved, moved_normals, k)
    F.check(ref_b, got_b, "moved sphere")
    print("rigid motion: %d of %d points compared" % (both.sum(), len(cloud)))
    assert both.sum() >= 0.5 * len(cloud)
    assert np.array_equal(got_a[1][both], got_b[1][both])
