"""GPU suite of mi_ndt_voxels, mi_ndt_register and mi_ndt_system against the float64 restatement of tests/ndt_reference.py.

The scenes are those of tests/test_gpu_plane.py ("origin" and "shifted": 4 000 fixed points on a sine surface, 3 000 of them moved by the
inverse of the ground truth G); the voxel map is mi_ndt_voxels' own of the fixed cloud at voxel 0.5 (78 voxels, 7 of them below 6 points).

The bounds (none of them taken from what the device gives):
  voxels       coordinates, counts and means equal mi_voxel_downsample's bit for bit.  The covariance before the floor within
               2^-24 |x| + (count + 8) 2^-53 sum |term| / (count - 1) of the restatement's about the SAME fp32 mean: the fp32 rounding, and
               the order of count additions of the same fp64 products.  icov6 (and cov6 under the default floor) within one fp32 unit of the
               restatement's largest entry of that voxel, 2^-23 max |M|: the fp64 differences between the Jacobi iteration and eigh are
               amplified by a condition number of at most 1 / eig_ratio = 100 and stay eight orders of magnitude below the fp32 grain, so
               they can only flip a rounding.
  sums         idx, terms, the centre and sums[28], sums[29] equal; every other sum within (n + 8) 2^-53 sum |term| + 3 2^-52 sum |term|,
               sum |term| formed by the restatement over every (point, voxel) term's own contribution: the order of the additions, and the
               exp -- the device's and glibc's fp64 exp are each within one unit of the last place of the true value on an identical
               argument (ROCm's device-library documentation, OCML: exp, double precision, 1 ULP), so e differs by 2 units at most, and the
               third unit is the product w = k e rounding differently behind it.
  one step     test_gpu_gicp.py's: every entry of out_T within 2^-23 max(1, |entry|) + 1e-12 cond(S) max(1, |c0|) of the restatement's
               step from the same fp32 pose; cond(S) <= 100 asserted.
  whole runs   max |dR| and max |dt| from the ground truth at most 4 x the restatement's own plus one fp32 unit of the largest entry; the
               iteration count within 2 of the restatement's.

An exact plane is NOT degenerate for this method: with the eigenvalue floor every voxel's matrix is positive definite, so sum H is
singular only when omega x P + v = 0 for every point, that is for collinear points.  The restatement and the device are held to the same
stop on the plane (both slide along it until MI_STOP_MAX_ITERATIONS), and MI_STOP_DEGENERATE with the pose untouched is shown on a line."""
import ctypes as C
import functools

import numpy as np
import pytest

import ndt_reference as N
import plane_reference as P
from test_gpu_plane import EPS_TRANSLATION, SCENES, bits, distance, frozen, moving_of, pose_of, scene

pytestmark = pytest.mark.gpu

VOXEL = 0.5
NEIGHBOURHOODS = (1, 7)
_maps = {}


def scene_map(ctx, name, voxel=VOXEL):
    """mi_ndt_voxels' map of the scene's fixed cloud, worked once"""
    if (name, voxel) not in _maps:
        _maps[name, voxel] = ctx.ndt_voxels(scene(name)[1], voxel)
    return _maps[name, voxel]


@functools.lru_cache(maxsize=None)
def reference_map(name, voxel=VOXEL):
    return N.voxels(scene(name)[1], voxel)


@functools.lru_cache(maxsize=None)
def reference_run(name, neighbourhood):
    return N.register(scene(name)[0], reference_map(name), 1e-6, EPS_TRANSLATION[name], 50, neighbourhood)


# ---- 1. the voxels' distributions
def check_voxels(ctx, cloud, voxel, origin, what, min_points=6, ratios=(1e-30, 0.01)):
    cloud = np.ascontiguousarray(cloud, np.float32)
    xyz, counts, coords = ctx.voxel_downsample(cloud, voxel, origin, want_counts=True, want_coords=True)
    for ratio in ratios:
        got = ctx.ndt_voxels(cloud, voxel, origin, min_points, ratio, want_cov=True)
        assert np.array_equal(got["coord"], coords) and np.array_equal(got["count"], counts) and np.array_equal(bits(got["mean"]), bits(xyz)), what
        want_origin = cloud.min(axis=0) if origin is None else np.asarray(origin, np.float32)
        assert np.array_equal(bits(got["origin"]), bits(want_origin)), what
        ref = N.voxels(cloud, voxel, origin, min_points, ratio, mean=got["mean"])
        assert np.array_equal(ref["coord"], coords) and np.array_equal(ref["count"], counts), what
        has = ref["has"]
        assert np.array_equal((got["icov"] != 0).any(axis=1), has), what
        assert (got["icov"][~has] == 0).all() and (got["cov"][~has] == 0).all(), what
        if not has.any():
            continue
        cnt = counts[has].astype(np.float64)[:, None]
        if ratio < 0.01:                     # no floor is active: cov6 is C itself
            assert not ref["raised"][has].any(), what
            bound = 2.0 ** -24 * np.abs(ref["C"][has]) + (cnt + 8) * 2.0 ** -53 * ref["C_abs"][has]
            err = np.abs(got["cov"][has].astype(np.float64) - ref["C"][has])
            print("%s: %d voxels, %d with a distribution; worst covariance error %.2e of its bound" % (what, len(counts), has.sum(), (err / np.maximum(bound, 1e-300)).max()))
            assert (err <= bound).all(), (what, err.max())
            continue                         # (without a floor M is as ill-conditioned as C: its bound below is for a ratio of 0.01)
        else:
            bound = 2.0 ** -23 * np.abs(ref["cov64"][has]).max(axis=1, keepdims=True)
            assert (np.abs(got["cov"][has].astype(np.float64) - ref["cov64"][has]) <= bound).all(), what
        bound = 2.0 ** -23 * np.abs(ref["M64"][has]).max(axis=1, keepdims=True)
        err = np.abs(got["icov"][has].astype(np.float64) - ref["M64"][has])
        assert (err <= bound).all(), (what, (err / bound).max())
    return got


@pytest.mark.parametrize("voxel", [0.5, 1.0])
@pytest.mark.parametrize("origin", [None, (3.1, 2.7, 1.3)])
def test_voxels_of_the_scene(ctx, voxel, origin):
    got = check_voxels(ctx, scene("origin")[1], voxel, origin, "scene voxel %g origin %s" % (voxel, origin))
    assert (voxel > 0.5 or (got["count"] < 6).any()) and (origin is None or (got["coord"] < 0).all())


@pytest.mark.parametrize("n", [1, 5, 6, 7, 257])
def test_voxels_of_small_clouds(ctx, n):
    cloud = scene("origin")[1][:n]
    check_voxels(ctx, cloud, 0.5, None, "n %d" % n)
    check_voxels(ctx, cloud, 100.0, (-50.0, -50.0, -50.0), "n %d in one voxel" % n)


def test_voxels_edge_cases(ctx):
    rng = np.random.default_rng(11)
    # one segment longer than a sums tile: 3 000 points in one voxel, between two small ones
    big = np.concatenate([rng.uniform(0.0, 0.4, (7, 3)), rng.uniform(0.0, 1.0, (3000, 3)) * [0.45, 0.45, 0.45] + [0.5, 0, 0], rng.uniform(1.0, 1.4, (9, 3))]).astype(np.float32)
    got = check_voxels(ctx, rng.permutation(big), 0.5, (0.0, 0.0, 0.0), "3000 in one voxel")
    assert got["count"].max() == 3000
    # a voxel of identical points: no distribution, but its row, count and mean
    same = np.concatenate([np.tile(np.array([[0.25, 0.25, 0.25]], np.float32), (10, 1)), rng.uniform(0.5, 1.0, (20, 3)).astype(np.float32)])
    got = check_voxels(ctx, same, 0.5, (0.0, 0.0, 0.0), "identical points")
    assert got["count"][0] == 10 and (got["icov"][0] == 0).all() and (got["icov"][1] != 0).any()
    # min_points decides (three points span a plane: only the floor makes their matrix invertible, so the default ratio alone)
    got = check_voxels(ctx, scene("origin")[1][:500], 0.5, None, "min_points 3", min_points=3, ratios=(0.01,))
    assert ((got["count"] >= 3) == (got["icov"] != 0).any(axis=1)).all()


# ---- 2. the lookup
@functools.lru_cache(maxsize=None)
def cube():
    rng = np.random.default_rng(23)
    cloud = rng.uniform(-5, 5, (20000, 3)).astype(np.float32)
    inside = rng.uniform(-5, 5, (5000, 3))
    inside[::3] += rng.choice([-12.0, 12.0], (len(inside[::3]), 3))           # a third of the queries outside the box
    return frozen(cloud), frozen(inside.astype(np.float32))


def test_lookup_against_the_dictionary(ctx):
    cloud, queries = cube()
    vox = ctx.ndt_voxels(cloud, 0.8, (0.3, 0.1, -0.2), 3, 0.01)
    has = (vox["icov"] != 0).any(axis=1)
    assert 1800 <= len(vox["coord"]) <= 2500 and (vox["coord"] < 0).any() and has.sum() > 1500
    holes = dict(vox, icov=vox["icov"].copy())
    holes["icov"][::5] = 0                                                        # rows without a distribution are never hit
    for label, m in (("full", vox), ("holes", holes), ("one row", {k: (v[700:701] if k in ("coord", "mean", "icov", "count") else v) for k, v in vox.items()})):
        lookup = N.Lookup(m)
        for nb in (1, 7, 27):
            ref = N.sums_at(queries, m, nb, lookup=lookup)
            sums, centre, idx, terms = ctx.ndt_system(queries, m, None, nb)
            assert np.array_equal(idx, ref["idx"]) and np.array_equal(terms, ref["terms"]), (label, nb)
            assert sums[28] == ref["sums"][28] and sums[29] == ref["sums"][29] and np.array_equal(bits(centre), bits(ref["centre"])), (label, nb)
            print("lookup %s neighbourhood %d: %d points with a term, %d terms" % (label, nb, sums[28], sums[29]))
            if label == "holes":
                assert not np.isin(idx[idx >= 0] % 5, [0]).any()
            if label == "full":
                assert (idx[::3] == -1).all() and (idx >= 0).sum() > 2500 and (nb == 1 or terms.max() > 1)


# ---- 3. one linearisation against the restatement, element by element
def assert_sums(sums, ref, n, what):
    want, mags = ref["sums"], ref["abs"]
    assert sums[28] == want[28] and sums[29] == want[29] and (sums[30:] == 0).all(), what
    bound = (n + 8) * 2.0 ** -53 * mags[:28] + 3 * 2.0 ** -52 * mags[:28]
    err = np.abs(sums[:28] - want[:28])
    print("%s: %d terms of %d points; worst sum error %.2e of its bound" % (what, int(sums[29]), int(sums[28]), (err[bound > 0] / bound[bound > 0]).max(initial=0.0)))
    assert (err <= bound).all(), (what, err, bound)


def check_system(ctx, moving, vox, T, nb, what):
    R, t = pose_of(T)
    ref = N.system(moving, vox, R, t, nb)
    sums, centre, idx, terms = ctx.ndt_system(moving, vox, T, nb)
    assert np.array_equal(idx, ref["idx"]) and np.array_equal(terms, ref["terms"]), what
    assert np.array_equal(bits(centre), bits(ref["centre"])), what
    assert_sums(sums, ref, len(moving), what)
    return sums, centre, idx, terms


@pytest.mark.parametrize("nb", NEIGHBOURHOODS)
@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 3000, 4097])
def test_ndt_system_sizes(ctx, n, name, nb):
    vox, Gt = scene_map(ctx, name), scene(name)[3]
    moving = moving_of(name, n)
    for label, T in (("null", None), ("truth", Gt.astype(np.float32))):
        first = check_system(ctx, moving, vox, T, nb, "%s n %d neighbourhood %d T %s" % (name, n, nb, label))
        again = ctx.ndt_system(moving, vox, T, nb)
        assert all(np.array_equal(bits(a) if a.dtype.kind == "f" else a, bits(b) if b.dtype.kind == "f" else b) for a, b in zip(first, again))
    a, b = ctx.ndt_system(moving, vox, None, nb), ctx.ndt_system(moving, vox, np.eye(4, dtype=np.float32), nb)
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])


def test_ndt_system_27(ctx):
    vox, Gt = scene_map(ctx, "origin"), scene("origin")[3]
    check_system(ctx, scene("origin")[0], vox, Gt.astype(np.float32), 27, "origin neighbourhood 27")


# ---- 4. beyond the rows one workgroup sums: three launches
def test_ndt_system_beyond_the_rows_one_workgroup_sums(ctx):
    fixed = scene("origin")[1]
    vox = scene_map(ctx, "origin")
    rng = np.random.default_rng(5)
    big = (fixed[rng.integers(0, 4000, 70000)] + rng.normal(0, 1e-3, (70000, 3))).astype(np.float32)
    first = check_system(ctx, big, vox, None, 7, "70000 points")
    again = ctx.ndt_system(big, vox, None, 7)
    assert np.array_equal(bits(first[0]), bits(again[0])) and np.array_equal(first[2], again[2]) and np.array_equal(first[3], again[3])
    assert first[0][28] > 60000


# ---- 5. one iteration from a given start
@pytest.mark.parametrize("nb", NEIGHBOURHOODS)
@pytest.mark.parametrize("name", SCENES)
def test_one_iteration_from_the_restatements_poses(ctx, capi, name, nb):
    moving = scene(name)[0]
    vox = scene_map(ctx, name)
    run = reference_run(name, nb)
    assert len(run["poses"]) >= 3
    c0 = np.abs(N.centre(vox)).max()
    for k, pose in enumerate(run["poses"][::3]):
        Tk = P.pose44(*pose)
        st = N.step(moving, vox, Tk[:3, :3].astype(np.float64), Tk[:3, 3].astype(np.float64), nb)
        assert st["stop"] is None and st["kappa"] <= 100, (name, k, st["kappa"])
        R, t, it, score, why = ctx.ndt_register(moving, vox, capi.ndt_params(max_iterations=1, neighbourhood=nb, eps_rotation=0.0, eps_translation=0.0), init=Tk)
        assert it == 1 and why == capi.STOP_MAX_ITERATIONS
        got, want = np.concatenate([R.ravel(), t]).astype(np.float64), np.concatenate([st["R"].ravel(), st["t"]])
        bound = 2.0 ** -23 * np.maximum(1, np.abs(want)) + 1e-12 * st["kappa"] * max(1.0, c0)
        print("%s neighbourhood %d step %d: cond(S) %.2f, worst entry %.2e of its bound, score %.4f" % (name, nb, 3 * k, st["kappa"], (np.abs(got - want) / bound).max(), score))
        assert (np.abs(got - want) <= bound).all(), (name, k, np.abs(got - want), bound)
        assert abs(np.float64(score) - np.float64(st["score"])) <= np.spacing(np.float32(st["score"])), (name, k, score, st["score"])


# ---- 6. whole registrations
@pytest.mark.parametrize("nb", NEIGHBOURHOODS)
@pytest.mark.parametrize("name", SCENES)
def test_whole_registration(ctx, capi, name, nb):
    moving, _, _, Gt = scene(name)
    vox = scene_map(ctx, name)
    assert np.array_equal(vox["coord"], reference_map(name)["coord"]) and np.array_equal(vox["count"], reference_map(name)["count"])
    run = reference_run(name, nb)
    assert run["stop"] == N.STOP_CONVERGED

    def go(**kw):
        R, t, it, score, why = ctx.ndt_register(moving, vox, capi.ndt_params(neighbourhood=nb, eps_translation=EPS_TRANSLATION[name], **kw))
        return R, t, it, score, why

    R, t, it, score, why = go()
    assert why == capi.STOP_CONVERGED
    dR, dt = distance(R, t, Gt)
    rR, rt = distance(run["R"], run["t"], Gt)
    print("%s neighbourhood %d: device %d iterations, |dR| %.2e |dt| %.2e, score %.4f; restatement %d iterations, |dR| %.2e |dt| %.2e, score %.4f" % (
        name, nb, it, dR, dt, score, run["iterations"], rR, rt, run["score"]))
    assert dR <= 4 * rR + np.spacing(np.float32(1.0))
    assert dt <= 4 * rt + np.spacing(np.float32(np.abs(Gt[:3, 3]).max()))
    assert abs(it - run["iterations"]) <= 2 and 0 < score <= 1
    first = (bits(R).tolist(), bits(t).tolist(), it, bits(np.float32(score)).tolist(), why)
    for sync_every in (1, 4, 50):
        R, t, it, score, why = go(sync_every=sync_every)
        assert (bits(R).tolist(), bits(t).tolist(), it, bits(np.float32(score)).tolist(), why) == first, sync_every


def test_the_other_outcomes(ctx, capi):
    moving = scene("origin")[0]
    vox = scene_map(ctx, "origin")
    start = P.pose44(P.rodrigues([0.0, 0.0, 0.01]), [0.01, 0.0, 0.0])
    # max_iterations = 0 returns init_T
    R, t, it, score, why = ctx.ndt_register(moving, vox, capi.ndt_params(max_iterations=0), init=start)
    assert (it, score, why) == (0, 0.0, capi.STOP_MAX_ITERATIONS)
    assert np.array_equal(bits(R), bits(start[:3, :3])) and np.array_equal(bits(t), bits(start[:3, 3]))
    R, t, it, score, why = ctx.ndt_register(moving, vox, capi.ndt_params(max_iterations=0))
    assert it == 0 and np.array_equal(R, np.eye(3, dtype=np.float32)) and np.array_equal(t, np.zeros(3, np.float32))
    # fewer than 6 terms reachable: five points with one voxel each; a cloud far from every listed voxel; a list without a distribution
    for cloud, m, nb in ((moving[:5], vox, 1), (moving + np.float32(40), vox, 27), (moving, dict(vox, icov=np.zeros_like(vox["icov"])), 7)):
        R, t, it, score, why = ctx.ndt_register(cloud, m, capi.ndt_params(neighbourhood=nb), init=start)
        assert (it, why) == (0, capi.STOP_NO_PAIRS) and np.array_equal(bits(R), bits(start[:3, :3])) and np.array_equal(bits(t), bits(start[:3, 3]))
    assert ctx.ndt_system(moving + np.float32(40), vox, None, 27)[0].tolist() == [0.0] * 32
    # collinear points: the rotation about the line is undetermined; the pose stays
    rng = np.random.default_rng(3)
    s = np.sort(rng.uniform(-2, 2, 500)).astype(np.float32)
    line = np.stack([s, np.zeros(500, np.float32), np.zeros(500, np.float32)], axis=1)
    lvox = ctx.ndt_voxels(line, 0.5, (-2.5, -0.25, -0.25))
    assert (lvox["icov"] != 0).any(axis=1).sum() >= 6
    for init in (None, np.eye(4, dtype=np.float32)):
        R, t, it, score, why = ctx.ndt_register(line[:300], lvox, capi.ndt_params(), init=init)
        assert (it, why) == (0, capi.STOP_DEGENERATE) and np.array_equal(R, np.eye(3, dtype=np.float32)) and np.array_equal(t, np.zeros(3, np.float32))
        assert N.step(line[:300], lvox, np.eye(3), np.zeros(3))["stop"] == N.STOP_DEGENERATE and 0 < score <= 1
    # an exact plane: the floor keeps every voxel's matrix positive definite, so the system is determined -- the restatement says which stop
    xy = rng.uniform(-2, 2, (4000, 2))
    plane = np.stack([xy[:, 0], xy[:, 1], np.zeros(4000)], axis=1).astype(np.float32)
    pvox = ctx.ndt_voxels(plane, 0.5, (-2.25, -2.25, -0.25))
    small = P.pose44(P.rodrigues([0.0, 0.0, 0.02]), [0.03, -0.02, 0.0])
    ref = N.register(plane[:3000], pvox, init=small)
    R, t, it, score, why = ctx.ndt_register(plane[:3000], pvox, capi.ndt_params(), init=small)
    print("exact plane: device stop %d after %d iterations, restatement stop %d after %d" % (why, it, ref["stop"], ref["iterations"]))
    assert why == ref["stop"] and abs(it - ref["iterations"]) <= 2


# ---- 7. refusals: nothing is written
def test_invalid_arguments_are_refused_with_the_outputs_untouched(ctx, capi):
    moving = scene("origin")[0][:200].copy()
    vox = scene_map(ctx, "origin")
    coord, mean, icov, origin = vox["coord"].copy(), vox["mean"].copy(), vox["icov"].copy(), vox["origin"].copy()
    n, nv = len(moving), len(coord)
    nan, inf = float("nan"), float("inf")

    def spoiled(a, row, value, col=1):
        a = a.copy()
        a[row, col] = value
        return a

    def register(what, before=moving, coord=coord, mean=mean, icov=icov, origin=origin, n=n, nv=nv, voxel=0.5, init=None, null=(), **kw):
        p = capi.ndt_params(**kw)
        T, it, score, why = np.full(16, -7.5, np.float32), C.c_int(-7), C.c_float(-7.5), C.c_int(-7)
        ptr = {"before": before.ctypes.data, "coord": coord.ctypes.data, "mean": mean.ctypes.data, "icov": icov.ctypes.data, "origin": origin.ctypes.data,
               "params": C.addressof(p), "out_T": T.ctypes.data}
        for k in null:
            ptr[k] = None
        rc = capi.ndt_register_raw(ctx._h, ptr["before"], n, ptr["coord"], ptr["mean"], ptr["icov"], nv, voxel, ptr["origin"], ptr["params"],
                                   None if init is None else init.ctypes.data, ptr["out_T"], C.addressof(it), C.addressof(score), C.addressof(why))
        msg = capi.lib().mi_last_error().decode()
        assert rc == capi.MI_ERR_INVALID_ARG and msg.startswith("mi_ndt_register"), (what, rc, msg)
        assert (T == -7.5).all() and it.value == -7 and score.value == -7.5 and why.value == -7, what
        return msg

    for k in ("before", "coord", "mean", "icov", "origin", "params", "out_T"):
        register("null " + k, null=(k,))
    register("n = 0", n=0)
    register("nv = 0", nv=0)
    for v in (0.0, -0.5, nan, inf):
        register("voxel %g" % v, voxel=v)
    register("origin", origin=np.array([0, nan, 0], np.float32))
    for v in (0.0, 1.0, -0.5, nan):
        register("outlier_ratio %g" % v, outlier_ratio=v)
    for v in (0, 2, 8, 26, -1):
        register("neighbourhood %d" % v, neighbourhood=v)
    register("eps_rotation negative", eps_rotation=-1e-3)
    register("eps_translation nan", eps_translation=nan)
    register("max_iterations", max_iterations=-1)
    register("sync_every", sync_every=-1)
    assert "before_xyz point 17" in register("before nan", before=spoiled(spoiled(moving, 17, nan), 150, nan))
    assert "before_xyz point 6" in register("before large", before=spoiled(moving, 6, 2e18))
    assert "vox_mean row 5 " in register("mean inf", mean=spoiled(spoiled(mean, 5, inf), 40, nan))
    assert "vox_icov6 row 11 " in register("icov nan", icov=spoiled(spoiled(icov, 11, nan, 5), 60, nan, 0))
    assert "vox_icov6 row 12 " in register("icov large", icov=spoiled(icov, 12, -2e18, 3))
    swapped = coord.copy()
    swapped[[20, 21]] = swapped[[21, 20]]
    assert "vox_coord row 21 " in register("unsorted", coord=swapped)
    twice = coord.copy()
    twice[31] = twice[30]
    assert "vox_coord row 31 " in register("duplicate", coord=twice)
    late = twice.copy()
    late[61] = late[60]
    assert "vox_coord row 31 " in register("two duplicates", coord=late)
    far = coord.copy()
    far[-1, 2] = 1 << 30
    assert "vox_coord row %d " % (nv - 1) in register("coordinate range", coord=far)
    wide = coord.copy()
    wide[-1, 2] = (1 << 20) + 5
    assert "span" in register("extent", coord=wide)
    bad = np.eye(4, dtype=np.float32).reshape(16)
    bad[13] = inf
    assert "entry 13" in register("transform", init=bad)

    def system(what, before=moving, coord=coord, icov=icov, T=None, nb=7, ratio=0.55, n=n, null_sums=False):
        sums, centre, idx, terms = np.full(32, -7.5), np.full(3, -7.5, np.float32), np.full(len(before), -7, np.int32), np.full(len(before), 77, np.uint8)
        rc = capi.ndt_system_raw(ctx._h, before.ctypes.data, n, coord.ctypes.data, mean.ctypes.data, icov.ctypes.data, nv, 0.5, origin.ctypes.data,
                                 None if T is None else T.ctypes.data, nb, ratio, None if null_sums else sums.ctypes.data, centre.ctypes.data, idx.ctypes.data,
                                 terms.ctypes.data)
        msg = capi.lib().mi_last_error().decode()
        assert rc == capi.MI_ERR_INVALID_ARG and msg.startswith("mi_ndt_system"), (what, rc, msg)
        assert (sums == -7.5).all() and (centre == -7.5).all() and (idx == -7).all() and (terms == 77).all(), what
        return msg

    system("n = 0", n=0)
    system("null sums", null_sums=True)
    system("neighbourhood", nb=3)
    system("ratio", ratio=1.5)
    assert "before_xyz point 3" in system("before nan", before=spoiled(moving, 3, nan))
    assert "vox_icov6 row 7 " in system("icov large", icov=spoiled(icov, 7, 1.5e18))
    assert "vox_coord row 21 " in system("unsorted", coord=swapped)
    system("transform", T=bad)

    def voxels(what, cloud=moving, n=n, voxel=0.5, origin=None, min_points=6, ratio=0.01, null=()):
        oc, om, oi = np.full((n or 1, 3), -7, np.int32), np.full((n or 1, 3), -7.5, np.float32), np.full((n or 1, 6), -7.5, np.float32)
        on, ocount, ocov, oo = C.c_int(-7), np.full(n or 1, -7, np.int32), np.full((n or 1, 6), -7.5, np.float32), np.full(3, -7.5, np.float32)
        ptr = {"xyz": cloud.ctypes.data, "coord": oc.ctypes.data, "mean": om.ctypes.data, "icov": oi.ctypes.data, "n": C.addressof(on)}
        for k in null:
            ptr[k] = None
        rc = capi.ndt_voxels_raw(ctx._h, ptr["xyz"], n, voxel, None if origin is None else origin.ctypes.data, min_points, ratio, ptr["coord"], ptr["mean"],
                                 ptr["icov"], ptr["n"], ocount.ctypes.data, ocov.ctypes.data, oo.ctypes.data)
        msg = capi.lib().mi_last_error().decode()
        assert rc == capi.MI_ERR_INVALID_ARG and msg.startswith("mi_ndt_voxels"), (what, rc, msg)
        assert (oc == -7).all() and (om == -7.5).all() and (oi == -7.5).all() and on.value == -7 and (ocount == -7).all() and (ocov == -7.5).all() and (oo == -7.5).all(), what
        return msg

    for k in ("xyz", "coord", "mean", "icov", "n"):
        voxels("null " + k, null=(k,))
    voxels("n = 0", n=0)
    voxels("voxel", voxel=-1.0)
    voxels("origin", origin=np.array([inf, 0, 0], np.float32))
    voxels("min_points", min_points=2)
    for v in (0.0, 1.5, nan):
        voxels("eig_ratio %g" % v, ratio=v)
    assert "point 9 " in voxels("nan", cloud=spoiled(spoiled(moving, 9, nan), 90, inf))
    assert "span" in voxels("extent", voxel=1e-7)
    # the context still works
    assert ctx.ndt_system(moving, vox)[0][29] > 0


# ---- 8. the contract
def test_a_loaded_icp_problem_survives(ctx, capi, bunny):
    before, after = bunny
    moving, fixed, _, _ = scene("origin")
    vox = scene_map(ctx, "origin")
    params = capi.icp_params(eps=1e-9, max_iterations=12)

    def icp(between):
        ctx.icp_load(before, after, params)
        ctx.icp_run(5)
        if between:
            ctx.ndt_voxels(fixed, 0.5)
            ctx.ndt_register(moving, vox, capi.ndt_params())
            ctx.ndt_system(moving, vox)
        ctx.icp_run(7)
        R, t, it, err, why = ctx.icp_result()
        return bits(R).tolist(), bits(t).tolist(), it, bits(np.float32(err)).tolist(), why

    assert icp(True) == icp(False)


def test_times_and_buffers(capi, ctx):
    moving, fixed, _, _ = scene("origin")
    start = capi.selftest_live_buffers()
    with capi.Context(0) as own:
        own.profile_enable(True)
        vox = own.ndt_voxels(fixed, 0.5)
        own.ndt_register(moving, vox, capi.ndt_params())
        times = own.ndt_times()
        assert times["total"] > 0 and times["iterations"] > 0 and all(v >= 0 for v in times.values())
        assert capi.selftest_live_buffers() > start
    assert capi.selftest_live_buffers() - start == 0
