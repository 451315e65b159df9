"""GPU suite of mi_icp_plane_register and mi_plane_system against the float64 restatement of tests/plane_reference.py.  The restatement's
O(n m) part, the k = 1 keys of tests/knn_reference.py, is worked once per scene and pose (lru_cache) and shared.

The scene: 4 000 fixed points on z = 0.3 sin(1.5 x) cos(1.2 y), x and y uniform in [-2, 2], with their analytic unit normals; the moving
cloud is 3 000 of them moved by the inverse of G, a rotation of 5 degrees about (1, 2, 3) through the centroid and a translation of
(0.05, -0.03, 0.04), so that G is the registration's ground truth.  "shifted" is the same scene moved by (100, -50, 25); there a
coordinate's fp32 grain is 8e-6, the updates stall at |v| of about 5e-6, and the scene is run with eps_translation = 1e-4.

The bounds (none of them taken from what the device gives):
  sums         idx, the centre and the pair count equal; every other sum within (n + 8) 2^-53 sum |term|, sum |term| formed by the
               restatement: the terms are the same float64 operations on both sides, so what differs is the order of n additions
  one step     every entry of out_T within 2^-23 max(1, |entry|) + 1e-12 cond(S) max(1, |c0|) of the restatement's step from the same
               fp32 pose: one fp32 unit for the double rounding, and the sums' bound carried through the solve; cond(S) <= 100 asserted
  whole runs   max |dR| and max |dt| from the ground truth at most 4 x the restatement's own plus one fp32 unit of the largest entry: once
               q differs in its last bit a few matches differ, which the factor allows for"""
import functools

import numpy as np
import pytest

import knn_reference as K
import plane_reference as P

pytestmark = pytest.mark.gpu

MODES = (K.DIST_CPU_ROUNDING, K.DIST_FMA)
SCENES = ("origin", "shifted")
LIMIT = 0.25
EPS_TRANSLATION = {"origin": 1e-6, "shifted": 1e-4}


def frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def scene(name):
    """(moving [3000, 3], fixed [4000, 3], normals [4000, 3], all float32; the ground truth G as a float64 [4, 4])"""
    rng = np.random.default_rng(97)
    xy = rng.uniform(-2, 2, (4000, 2))
    x, y = xy[:, 0], xy[:, 1]
    fixed = np.stack([x, y, 0.3 * np.sin(1.5 * x) * np.cos(1.2 * y)], axis=1)
    normals = np.stack([-0.45 * np.cos(1.5 * x) * np.cos(1.2 * y), 0.36 * np.sin(1.5 * x) * np.sin(1.2 * y), np.ones(4000)], axis=1)
    normals /= np.linalg.norm(normals, axis=1, keepdims=True)
    if name == "shifted":
        fixed = fixed + np.array([100.0, -50.0, 25.0])
    fixed = fixed.astype(np.float32)
    pick = rng.permutation(4000)[:3000]
    Rg = P.rodrigues(np.deg2rad(5.0) * np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0))
    c = fixed.astype(np.float64).mean(axis=0)
    G = np.eye(4)
    G[:3, :3], G[:3, 3] = Rg, c + np.array([0.05, -0.03, 0.04]) - Rg @ c
    moving = (fixed[pick].astype(np.float64) - G[:3, 3]) @ Rg                 # G^-1 p = Rg^T (p - t), row vectors
    return frozen(moving.astype(np.float32)), frozen(fixed), frozen(normals.astype(np.float32)), frozen(G)


def pose_of(T):
    return (np.eye(3), np.zeros(3)) if T is None else (np.asarray(T, np.float64)[:3, :3], np.asarray(T, np.float64)[:3, 3])


@functools.lru_cache(maxsize=None)
def reference_run(name, mode, max_iterations=50):
    moving, fixed, normals, _ = scene(name)
    return P.register(moving, fixed, normals, 1e-6, EPS_TRANSLATION[name], max_iterations, LIMIT, mode)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def check_system(ctx, moving, fixed, normals, T, mode, max_d2, what):
    """Test 1's comparison of one mi_plane_system call; returns the device's answer"""
    R, t = pose_of(T)
    ref = P.system(moving, fixed, normals, R, t, mode, max_d2)
    sums, centre, idx = ctx.plane_system(moving, fixed, normals, T, mode, max_d2)
    assert np.array_equal(idx, ref["idx"]), what
    assert np.array_equal(bits(centre), bits(ref["centre"])), what
    assert sums[29] == ref["sums"][29] and (sums[30:] == 0).all(), what
    bound = (len(moving) + 8) * 2.0 ** -53 * ref["abs"][:29]
    err = np.abs(sums[:29] - ref["sums"][:29])
    print("%s: %d pairs; worst sum error %.2e of its bound" % (what, int(sums[29]), (err[bound > 0] / bound[bound > 0]).max(initial=0.0)))
    assert (err <= bound).all(), (what, err, bound)
    return sums, centre, idx


def moving_of(name, n):
    """the scene's first n moving points; beyond its 3 000, copies of them 1e-3 off"""
    moving = scene(name)[0]
    if n <= len(moving):
        return moving[:n]
    rng = np.random.default_rng(5)
    extra = n - len(moving)
    return np.concatenate([moving, (moving[rng.integers(0, len(moving), extra)] + rng.normal(0, 1e-3, (extra, 3))).astype(np.float32)])


# ---- 1. one linearisation against the restatement, element by element
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 3000, 4097])
def test_plane_system_sizes(ctx, n, name, mode):
    _, fixed, normals, G = scene(name)
    for label, T in (("null", None), ("truth", G.astype(np.float32))):
        check_system(ctx, moving_of(name, n), fixed, normals, T, mode, LIMIT, "%s n %d mode %d T %s" % (name, n, mode, label))


@pytest.mark.parametrize("mode", MODES)
def test_plane_system_beyond_the_rows_one_workgroup_sums(ctx, mode):
    """70 000 moving points are 1 094 rows, beyond what the solve's workgroup sums itself: the slabs come first (three launches).  A
    restatement of the matches would cost n m here, so the device's matches are held to mi_knn_search's, bit for bit, and all 29 sums to
    the restatement's float64 terms of those pairs, under the bound of every other case."""
    _, fixed, normals, _ = scene("origin")
    rng = np.random.default_rng(5)
    big = (fixed[rng.integers(0, 4000, 70000)] + rng.normal(0, 1e-3, (70000, 3))).astype(np.float32)
    sums, centre, idx = ctx.plane_system(big, fixed, normals, None, mode, LIMIT)
    again = ctx.plane_system(big, fixed, normals, None, mode, LIMIT)
    assert np.array_equal(bits(sums), bits(again[0])) and np.array_equal(idx, again[2])
    kidx, kd2 = ctx.knn_search(big, fixed, 1, mode, LIMIT)
    assert np.array_equal(idx, kidx[:, 0]) and sums[29] == 70000 and (sums[30:] == 0).all()
    want, mags = P.sums_of_pairs(P.move_f32(np.eye(3), np.zeros(3), big), fixed, normals, idx, kd2[:, 0])
    bound = (70000 + 8) * 2.0 ** -53 * mags[:29]
    err = np.abs(sums[:29] - want[:29])
    print("70000 points mode %d: worst sum error %.2e of its bound" % (mode, (err / bound).max()))
    assert (err <= bound).all(), (err, bound)


@pytest.mark.parametrize("mode", MODES)
def test_plane_system_edge_cases(ctx, mode):
    moving, fixed, normals, G = scene("origin")
    Gf = G.astype(np.float32)
    # T NULL and the identity: the same bits
    a = ctx.plane_system(moving, fixed, normals, None, mode, LIMIT)
    b = ctx.plane_system(moving, fixed, normals, np.eye(4, dtype=np.float32), mode, LIMIT)
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[2], b[2]) and np.array_equal(bits(a[1]), bits(b[1]))
    check_system(ctx, moving, fixed, normals, np.eye(4, dtype=np.float32), mode, LIMIT, "identity mode %d" % mode)
    # a limit that drops about half the pairs (the start is 5 degrees off: the median match distance decides)
    d2 = K.unpack(K.sorted_keys(P.move_f32(np.eye(3), np.zeros(3), moving), fixed, mode, keep=1), 1)[1][:, 0]
    sums, _, idx = check_system(ctx, moving, fixed, normals, None, mode, float(np.median(d2)), "half the pairs mode %d" % mode)
    assert 1400 <= sums[29] <= 1600 and (idx == -1).sum() == 3000 - sums[29]
    # 5 % of the normals zero
    holes = normals.copy()
    holes[np.random.default_rng(7).permutation(4000)[:200]] = 0
    sums, _, idx = check_system(ctx, moving, fixed, holes, Gf, mode, LIMIT, "zero normals mode %d" % mode)
    assert 0 < (idx == -1).sum() < 400
    # moving points outside the fixed cloud's box, with and without a limit
    out = (moving + np.array([3.0, -2.5, 6.0], np.float32)).astype(np.float32)
    check_system(ctx, out[:500], fixed, normals, None, mode, np.inf, "outside mode %d" % mode)
    sums, _, idx = check_system(ctx, out[:500], fixed, normals, None, mode, LIMIT, "outside, limited mode %d" % mode)
    assert sums[29] == 0 and (idx == -1).all()
    # m = 1
    check_system(ctx, moving[:100], fixed[:1], normals[:1], Gf, mode, np.inf, "m = 1 mode %d" % mode)
    # the shifted scene from the identity
    moving, fixed, normals, G = scene("shifted")
    check_system(ctx, moving, fixed, normals, None, mode, LIMIT, "shifted identity mode %d" % mode)


# ---- 2. one iteration from a given start
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", SCENES)
def test_one_iteration_from_the_restatements_poses(ctx, capi, name, mode):
    moving, fixed, normals, _ = scene(name)
    run = reference_run(name, mode)
    assert len(run["poses"]) >= 3
    c0 = np.abs(P.centre(fixed)).max()
    for k in range(3):
        Tk = P.pose44(*run["poses"][k])
        st = P.step(moving, fixed, normals, Tk[:3, :3].astype(np.float64), Tk[:3, 3].astype(np.float64), mode, LIMIT)
        assert st["stop"] is None and st["kappa"] <= 100, (name, k, st["kappa"])
        R, t, it, err, why = ctx.icp_plane_register(moving, fixed, normals, capi.plane_params(max_iterations=1, max_distance_squared=LIMIT, dist_mode=mode,
                                                                                               eps_rotation=0.0, eps_translation=0.0), init=Tk)
        assert it == 1 and why == capi.STOP_MAX_ITERATIONS
        got, want = np.concatenate([R.ravel(), t]).astype(np.float64), np.concatenate([st["R"].ravel(), st["t"]])
        bound = 2.0 ** -23 * np.maximum(1, np.abs(want)) + 1e-12 * st["kappa"] * max(1.0, c0)
        print("%s mode %d step %d: cond(S) %.2f, worst entry %.2e of its bound, error %.3e" % (name, mode, k, st["kappa"], (np.abs(got - want) / bound).max(), err))
        assert (np.abs(got - want) <= bound).all(), (name, k, np.abs(got - want), bound)
        assert abs(np.float64(err) - np.float64(st["error"])) <= np.spacing(np.float32(st["error"])), (name, k, err, st["error"])


# ---- 3. whole registrations
def distance(R, t, G):
    return np.abs(np.asarray(R, np.float64) - G[:3, :3]).max(), np.abs(np.asarray(t, np.float64) - G[:3, 3]).max()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", SCENES)
def test_whole_registration_reaches_the_ground_truth(ctx, capi, name, mode):
    moving, fixed, normals, G = scene(name)
    run = reference_run(name, mode)
    assert run["stop"] == P.STOP_CONVERGED
    R, t, it, err, why = ctx.icp_plane_register(moving, fixed, normals, capi.plane_params(max_distance_squared=LIMIT, dist_mode=mode,
                                                                                           eps_translation=EPS_TRANSLATION[name]))
    assert why == capi.STOP_CONVERGED
    dR, dt = distance(R, t, G)
    rR, rt = distance(run["R"], run["t"], G)
    print("%s mode %d: device %d iterations, |dR| %.2e |dt| %.2e, error %.3e; restatement %d iterations, |dR| %.2e |dt| %.2e" % (
        name, mode, it, dR, dt, err, run["iterations"], rR, rt))
    assert dR <= 4 * rR + np.spacing(np.float32(1.0))
    assert dt <= 4 * rt + np.spacing(np.float32(np.abs(G[:3, 3]).max()))


def test_the_other_outcomes(ctx, capi):
    moving, fixed, normals, G = scene("origin")
    start = P.pose44(P.rodrigues([0.0, 0.0, 0.01]), [0.01, 0.0, 0.0])
    R, t, it, err, why = ctx.icp_plane_register(moving, fixed, normals, capi.plane_params(max_iterations=0, max_distance_squared=LIMIT), init=start)
    assert (it, err, why) == (0, 0.0, capi.STOP_MAX_ITERATIONS)
    assert np.array_equal(bits(R), bits(start[:3, :3])) and np.array_equal(bits(t), bits(start[:3, 3]))
    R, t, it, err, why = ctx.icp_plane_register(moving, fixed, normals, capi.plane_params(max_iterations=0))
    assert it == 0 and np.array_equal(R, np.eye(3, dtype=np.float32)) and np.array_equal(t, np.zeros(3, np.float32))
    R, t, it, err, why = ctx.icp_plane_register(moving, fixed, normals, capi.plane_params(max_iterations=2, max_distance_squared=LIMIT))
    assert (it, why) == (2, capi.STOP_MAX_ITERATIONS)
    ref = reference_run("origin", K.DIST_CPU_ROUNDING, 2)
    assert np.abs(R - ref["R"]).max() <= 1e-6 and np.abs(t - ref["t"]).max() <= 1e-6
    # separated clouds under a limit of 1e-12: no pair at all
    R, t, it, err, why = ctx.icp_plane_register(moving + np.float32(10), fixed, normals, capi.plane_params(max_distance_squared=1e-12), init=start)
    assert (it, err, why) == (0, 0.0, capi.STOP_NO_PAIRS) and np.array_equal(bits(R), bits(start[:3, :3])) and np.array_equal(bits(t), bits(start[:3, 3]))
    # an exact plane with +z normals determines three motions of six
    rng = np.random.default_rng(3)
    plane = np.concatenate([rng.uniform(-2, 2, (500, 2)), np.zeros((500, 1))], axis=1).astype(np.float32)
    up = np.tile(np.array([0, 0, 1], np.float32), (500, 1))
    R, t, it, err, why = ctx.icp_plane_register(plane[:300] + np.array([0, 0, 0.1], np.float32), plane, up, capi.plane_params(), init=start)
    assert (it, why) == (0, capi.STOP_DEGENERATE) and np.array_equal(bits(R), bits(start[:3, :3])) and np.array_equal(bits(t), bits(start[:3, 3]))
    assert abs(err - 0.01) <= 1e-6


# ---- 4. the contract
def test_same_bits_whatever_ran_before_and_whatever_the_batch(ctx, capi):
    moving, fixed, normals, _ = scene("origin")

    def run(**kw):
        R, t, it, err, why = ctx.icp_plane_register(moving, fixed, normals, capi.plane_params(max_distance_squared=LIMIT, **kw))
        return bits(R).tolist(), bits(t).tolist(), it, bits(np.float32(err)).tolist(), why

    first = run()
    assert run() == first
    ctx.knn_search(None, fixed, 8)
    ctx.estimate_normals(fixed, 8)
    ctx.remove_outliers(fixed, capi.outlier_params(k=8))
    assert run() == first
    for sync_every in (1, 3, 0):
        assert run(sync_every=sync_every) == first
    ctx.profile_enable(True)
    try:
        assert run() == first
        times = ctx.icp_plane_times()
    finally:
        ctx.profile_enable(False)
    assert times["total"] > 0 and times["iterations"] > 0 and all(v >= 0 for v in times.values())


def test_a_loaded_icp_problem_survives(ctx, capi, bunny):
    before, after = bunny
    moving, fixed, normals, _ = scene("origin")
    params = capi.icp_params(eps=1e-9, max_iterations=12)

    def icp(between):
        ctx.icp_load(before, after, params)
        ctx.icp_run(5)
        if between:
            ctx.icp_plane_register(moving, fixed, normals, capi.plane_params(max_distance_squared=LIMIT))
            ctx.plane_system(moving, fixed, normals)
        ctx.icp_run(7)
        R, t, it, err, why = ctx.icp_result()
        return bits(R).tolist(), bits(t).tolist(), it, bits(np.float32(err)).tolist(), why

    assert icp(True) == icp(False)


def test_estimated_normals_still_converge(ctx, capi):
    moving, fixed, _, _ = scene("origin")
    estimated = ctx.estimate_normals(fixed, 16)
    why = ctx.icp_plane_register(moving, fixed, estimated, capi.plane_params(max_distance_squared=LIMIT))[4]
    assert why == capi.STOP_CONVERGED


def test_invalid_arguments_are_refused_with_the_outputs_untouched(ctx, capi):
    import ctypes as C
    moving, fixed, normals, _ = scene("origin")
    moving, fixed, normals = moving[:200].copy(), fixed[:300].copy(), normals[:300].copy()
    n, m = len(moving), len(fixed)
    nan, inf = float("nan"), float("inf")

    def spoiled(a, row, value):
        a = a.copy()
        a[row, 1] = value
        return a

    def register(what, before=moving, after=fixed, nrm=normals, n=n, m=m, init=None, null=(), **kw):
        p = capi.plane_params(**kw)
        T, it, err, why = np.full(16, -7.5, np.float32), C.c_int(-7), C.c_float(-7.5), C.c_int(-7)
        ptr = {"before": before.ctypes.data, "after": after.ctypes.data, "normals": nrm.ctypes.data, "params": C.addressof(p), "out_T": T.ctypes.data}
        for k in null:
            ptr[k] = None
        rc = capi.icp_plane_register_raw(ctx._h, ptr["before"], n, ptr["after"], ptr["normals"], m, ptr["params"], None if init is None else init.ctypes.data,
                                         ptr["out_T"], C.addressof(it), C.addressof(err), C.addressof(why))
        msg = capi.lib().mi_last_error().decode()
        assert rc == capi.MI_ERR_INVALID_ARG and msg.startswith("mi_icp_plane_register"), (what, rc, msg)
        assert (T == -7.5).all() and it.value == -7 and err.value == -7.5 and why.value == -7, what
        return msg

    for k in ("before", "after", "normals", "params", "out_T"):
        register("null " + k, null=(k,))
    register("n = 0", n=0)
    register("m = 0", m=0)
    register("dist_mode", dist_mode=2)
    register("limit nan", max_distance_squared=nan)
    register("limit negative", max_distance_squared=-1.0)
    register("eps_rotation negative", eps_rotation=-1e-3)
    register("eps_translation nan", eps_translation=nan)
    register("max_iterations", max_iterations=-1)
    assert "before_xyz point 17" in register("before nan", before=spoiled(moving, 17, nan))
    assert "after_xyz point 5" in register("after inf", after=spoiled(fixed, 5, inf))
    assert "after_xyz point 6" in register("after large", after=spoiled(fixed, 6, 2e18))
    assert "after_normals_xyz normal 9" in register("normal nan", nrm=spoiled(normals, 9, nan))
    bad = np.eye(4, dtype=np.float32).reshape(16)
    bad[13] = inf
    assert "entry 13" in register("transform", init=bad)

    def system(what, before=moving, T=None, mode=0, max_d2=inf, n=n):
        sums, centre, idx = np.full(32, -7.5), np.full(3, -7.5, np.float32), np.full(len(before), -7, np.int32)
        rc = capi.plane_system_raw(ctx._h, before.ctypes.data, n, fixed.ctypes.data, normals.ctypes.data, m, None if T is None else T.ctypes.data, mode, max_d2,
                                   sums.ctypes.data, centre.ctypes.data, idx.ctypes.data)
        msg = capi.lib().mi_last_error().decode()
        assert rc == capi.MI_ERR_INVALID_ARG and msg.startswith("mi_plane_system"), (what, rc, msg)
        assert (sums == -7.5).all() and (centre == -7.5).all() and (idx == -7).all(), what

    system("n = 0", n=0)
    system("dist_mode", mode=7)
    system("limit", max_d2=-0.5)
    system("before nan", before=spoiled(moving, 3, nan))
    system("transform", T=bad)
    # the bottom row of a transform is never read, so nothing in it is refused; and the context still works
    loose = np.eye(4, dtype=np.float32)
    loose[3] = nan
    assert np.array_equal(bits(ctx.plane_system(moving, fixed, normals, loose)[0]), bits(ctx.plane_system(moving, fixed, normals)[0]))
    assert ctx.plane_system(moving, fixed, normals)[0][29] > 0


def test_no_buffer_outlives_its_context(capi, ctx):
    """(the session's context keeps its own buffers: the count goes back to where it was, 0 of this context's left)"""
    moving, fixed, normals, _ = scene("origin")
    start = capi.selftest_live_buffers()
    with capi.Context(0) as own:
        own.profile_enable(True)
        own.icp_plane_register(moving, fixed, normals, capi.plane_params(max_distance_squared=LIMIT))
        own.plane_system(moving, fixed, normals)
        assert capi.selftest_live_buffers() > start
    assert capi.selftest_live_buffers() - start == 0
