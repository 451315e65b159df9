"""GPU suite of mi_icp_gicp_register and mi_gicp_system against the float64 restatement of tests/gicp_reference.py.  The restatement's
O(n m) part, the k = 1 keys of tests/knn_reference.py, is worked once per scene and pose (lru_cache) and shared.

The scenes are those of tests/test_gpu_plane.py ("origin" and "shifted": 4 000 fixed points on a sine surface, 3 000 of them moved by the
inverse of the ground truth G).  The covariances are analytic: I - (1 - 1e-3) n n^T from the surface's analytic unit normals in float64,
rounded to float32; the moving cloud's from the same normals turned by G^-1.

The bounds (none of them taken from what the device gives):
  sums         idx, the centre and the pair count equal; every other sum within (n + 8) 2^-53 sum |term|, sum |term| formed by the
               restatement: the terms are the same float64 operations on both sides -- products, sums, differences and IEEE divisions, no
               libm call -- so what differs is the order of n additions
  one step     every entry of out_T within 2^-23 max(1, |entry|) + 1e-12 cond(S) max(1, |c0|) of the restatement's step from the same
               fp32 pose: one fp32 unit for the double rounding, and the sums' bound carried through the solve; cond(S) <= 1e4 asserted
  whole runs   max |dR| and max |dt| from the ground truth at most 4 x the restatement's own plus one fp32 unit of the largest entry; the
               iteration count within 2 of the restatement's: once q differs in its last bit a few matches differ"""
import ctypes as C
import functools

import numpy as np
import pytest

import gicp_reference as G
import knn_reference as K
import plane_reference as P
from test_gpu_plane import EPS_TRANSLATION, LIMIT, MODES, SCENES, bits, distance, frozen, pose_of, scene

pytestmark = pytest.mark.gpu

EPS = 1e-3
IDENTITY6 = np.array([1, 0, 0, 1, 0, 1], np.float32)


def plane_cov(normals64):
    return G.plane_covariance(normals64, EPS).astype(np.float32)


@functools.lru_cache(maxsize=None)
def gscene(name):
    """(moving [3000, 3], cov_b [3000, 6], fixed [4000, 3], cov_a [4000, 6], all float32; G float64 [4, 4]; the analytic normals float64)"""
    moving, fixed, _, Gt = scene(name)
    rng = np.random.default_rng(97)                        # the scene's own draws, again: the analytic normals in float64 and the pick
    xy = rng.uniform(-2, 2, (4000, 2))
    x, y = xy[:, 0], xy[:, 1]
    normals = np.stack([-0.45 * np.cos(1.5 * x) * np.cos(1.2 * y), 0.36 * np.sin(1.5 * x) * np.sin(1.2 * y), np.ones(4000)], axis=1)
    normals /= np.linalg.norm(normals, axis=1, keepdims=True)
    pick = rng.permutation(4000)[:3000]
    assert np.array_equal(((fixed[pick].astype(np.float64) - Gt[:3, 3]) @ Gt[:3, :3]).astype(np.float32), moving)
    moved_normals = normals[pick] @ Gt[:3, :3]             # G^-1's rotation, row vectors
    return moving, frozen(plane_cov(moved_normals)), fixed, frozen(plane_cov(normals)), Gt, frozen(normals)


def moving_of(name, n):
    """the scene's first n moving points and covariances; beyond its 3 000, copies of them 1e-3 off with the covariance of the original"""
    moving, cov_b = gscene(name)[:2]
    if n <= len(moving):
        return moving[:n], cov_b[:n]
    rng = np.random.default_rng(5)
    src = rng.integers(0, len(moving), n - len(moving))
    extra = (moving[src] + rng.normal(0, 1e-3, (len(src), 3))).astype(np.float32)
    return np.concatenate([moving, extra]), np.concatenate([cov_b, cov_b[src]])


@functools.lru_cache(maxsize=None)
def reference_run(name, mode, max_iterations=50):
    moving, cov_b, fixed, cov_a, _, _ = gscene(name)
    return G.register(moving, cov_b, fixed, cov_a, 1e-6, EPS_TRANSLATION[name], max_iterations, LIMIT, mode)


def assert_sums(sums, want, mags, n, what):
    assert sums[29] == want[29] and (sums[30:] == 0).all(), what
    bound = (n + 8) * 2.0 ** -53 * mags[:29]
    err = np.abs(sums[:29] - want[:29])
    print("%s: %d pairs; worst sum error %.2e of its bound" % (what, int(sums[29]), (err[bound > 0] / bound[bound > 0]).max(initial=0.0)))
    assert (err <= bound).all(), (what, err, bound)


def check_system(ctx, moving, cov_b, fixed, cov_a, T, mode, max_d2, what):
    """Test 1's comparison of one mi_gicp_system call; returns the device's answer"""
    R, t = pose_of(T)
    ref = G.system(moving, cov_b, fixed, cov_a, R, t, mode, max_d2)
    sums, centre, idx = ctx.gicp_system(moving, cov_b, fixed, cov_a, T, mode, max_d2)
    assert np.array_equal(idx, ref["idx"]), what
    assert np.array_equal(bits(centre), bits(ref["centre"])), what
    assert_sums(sums, ref["sums"], ref["abs"], len(moving), what)
    return sums, centre, idx


# ---- 1. one linearisation against the restatement, element by element
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 3000, 4097])
def test_gicp_system_sizes(ctx, n, name, mode):
    _, _, fixed, cov_a, Gt, _ = gscene(name)
    moving, cov_b = moving_of(name, n)
    for label, T in (("null", None), ("truth", Gt.astype(np.float32))):
        check_system(ctx, moving, cov_b, fixed, cov_a, T, mode, LIMIT, "%s n %d mode %d T %s" % (name, n, mode, label))


# ---- 2. beyond the rows one workgroup sums: three launches
@pytest.mark.parametrize("mode", MODES)
def test_gicp_system_beyond_the_rows_one_workgroup_sums(ctx, mode):
    """70 000 moving points are 1 094 rows: the slabs come first.  A restatement of the matches would cost n m here, so the device's matches
    are held to mi_knn_search's, bit for bit, and all 29 sums to the restatement's float64 terms of those pairs, under the bound of every
    other case."""
    _, _, fixed, cov_a, _, _ = gscene("origin")
    rng = np.random.default_rng(5)
    src = rng.integers(0, 4000, 70000)
    big, cov_b = (fixed[src] + rng.normal(0, 1e-3, (70000, 3))).astype(np.float32), np.ascontiguousarray(cov_a[src])
    sums, centre, idx = ctx.gicp_system(big, cov_b, fixed, cov_a, None, mode, LIMIT)
    again = ctx.gicp_system(big, cov_b, fixed, cov_a, None, mode, LIMIT)
    assert np.array_equal(bits(sums), bits(again[0])) and np.array_equal(idx, again[2])
    kidx, kd2 = ctx.knn_search(big, fixed, 1, mode, LIMIT)
    assert np.array_equal(idx, kidx[:, 0]) and sums[29] == 70000
    want, mags, ridx = G.sums_of_pairs(P.move_f32(np.eye(3), np.zeros(3), big), fixed, cov_b, cov_a, np.eye(3), idx, kd2[:, 0])
    assert np.array_equal(ridx, idx)
    assert_sums(sums, want, mags, 70000, "70000 points mode %d" % mode)


# ---- 3. edge cases
@pytest.mark.parametrize("mode", MODES)
def test_gicp_system_edge_cases(ctx, capi, mode):
    moving, cov_b, fixed, cov_a, Gt, _ = gscene("origin")
    Gf = Gt.astype(np.float32)
    # T NULL and the identity: the same bits
    a = ctx.gicp_system(moving, cov_b, fixed, cov_a, None, mode, LIMIT)
    b = ctx.gicp_system(moving, cov_b, fixed, cov_a, np.eye(4, dtype=np.float32), mode, LIMIT)
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[2], b[2]) and np.array_equal(bits(a[1]), bits(b[1]))
    # both covariances zero: no pair; one of them zero: the pair stays (point to distribution)
    rng = np.random.default_rng(7)
    holes_a, holes_b = cov_a.copy(), cov_b.copy()
    holes_a[rng.permutation(4000)[:800]] = 0
    holes_b[rng.permutation(3000)[:900]] = 0
    sums, _, idx = check_system(ctx, moving, holes_b, fixed, holes_a, Gf, mode, LIMIT, "zero covariances mode %d" % mode)
    full = ctx.gicp_system(moving, cov_b, fixed, cov_a, Gf, mode, LIMIT)[2]
    both = (holes_b == 0).all(axis=1) & (full >= 0) & (holes_a[np.maximum(full, 0)] == 0).all(axis=1)
    assert both.sum() > 50 and np.array_equal(idx == -1, both | (full == -1))
    sums, _, idx = check_system(ctx, moving, np.zeros_like(cov_b), fixed, cov_a, Gf, mode, LIMIT, "moving covariances zero mode %d" % mode)
    assert np.array_equal(idx, full)
    sums, _, idx = check_system(ctx, moving, cov_b, fixed, np.zeros_like(cov_a), Gf, mode, LIMIT, "fixed covariances zero mode %d" % mode)
    assert np.array_equal(idx, full)
    sums, _, idx = check_system(ctx, moving, np.zeros_like(cov_b), fixed, np.zeros_like(cov_a), Gf, mode, LIMIT, "all zero mode %d" % mode)
    assert sums[29] == 0 and (idx == -1).all() and (sums == 0).all()
    R, t, it, err, why = ctx.icp_gicp_register(moving, np.zeros_like(cov_b), fixed, np.zeros_like(cov_a), capi.plane_params(dist_mode=mode), init=Gf)
    assert (it, err, why) == (0, 0.0, capi.STOP_NO_PAIRS) and np.array_equal(bits(R), bits(Gf[:3, :3])) and np.array_equal(bits(t), bits(Gf[:3, 3]))
    # a limit that excludes everything
    out = (moving + np.array([3.0, -2.5, 6.0], np.float32)).astype(np.float32)
    check_system(ctx, out[:500], cov_b[:500], fixed, cov_a, None, mode, np.inf, "outside mode %d" % mode)
    sums, _, idx = check_system(ctx, out[:500], cov_b[:500], fixed, cov_a, None, mode, LIMIT, "outside, limited mode %d" % mode)
    assert sums[29] == 0 and (idx == -1).all()
    R, t, it, err, why = ctx.icp_gicp_register(moving + np.float32(10), cov_b, fixed, cov_a, capi.plane_params(max_distance_squared=1e-12, dist_mode=mode), init=Gf)
    assert (it, err, why) == (0, 0.0, capi.STOP_NO_PAIRS) and np.array_equal(bits(R), bits(Gf[:3, :3])) and np.array_equal(bits(t), bits(Gf[:3, 3]))
    # m = 1, and the shifted scene from the identity
    check_system(ctx, moving[:100], cov_b[:100], fixed[:1], cov_a[:1], Gf, mode, np.inf, "m = 1 mode %d" % mode)
    moving, cov_b, fixed, cov_a, _, _ = gscene("shifted")
    check_system(ctx, moving, cov_b, fixed, cov_a, None, mode, LIMIT, "shifted identity mode %d" % mode)


def test_the_other_outcomes(ctx, capi):
    moving, cov_b, fixed, cov_a, _, _ = gscene("origin")
    start = P.pose44(P.rodrigues([0.0, 0.0, 0.01]), [0.01, 0.0, 0.0])
    # collinear points with identity covariances: the rotation about the line is undetermined; the pose stays
    rng = np.random.default_rng(3)
    s = np.sort(rng.uniform(-2, 2, 500)).astype(np.float32)
    line = np.stack([s, np.zeros(500, np.float32), np.zeros(500, np.float32)], axis=1)
    eye_a, eye_b = np.tile(IDENTITY6, (500, 1)), np.tile(IDENTITY6, (300, 1))
    R, t, it, err, why = ctx.icp_gicp_register(line[:300], eye_b, line, eye_a, capi.plane_params())
    assert (it, why) == (0, capi.STOP_DEGENERATE) and np.array_equal(R, np.eye(3, dtype=np.float32)) and np.array_equal(t, np.zeros(3, np.float32))
    assert err == 0.0
    lifted = line[:300] + np.array([0, 0.1, 0], np.float32)
    R, t, it, err, why = ctx.icp_gicp_register(lifted, eye_b, line, eye_a, capi.plane_params(), init=np.eye(4, dtype=np.float32))
    assert (it, why) == (0, capi.STOP_DEGENERATE) and np.array_equal(R, np.eye(3, dtype=np.float32)) and np.array_equal(t, np.zeros(3, np.float32))
    assert abs(err - 0.005) <= 1e-6                       # Sigma = 2 I: e = |d|^2 / 2
    # max_iterations = 0
    R, t, it, err, why = ctx.icp_gicp_register(moving, cov_b, fixed, cov_a, capi.plane_params(max_iterations=0, max_distance_squared=LIMIT), init=start)
    assert (it, err, why) == (0, 0.0, capi.STOP_MAX_ITERATIONS)
    assert np.array_equal(bits(R), bits(start[:3, :3])) and np.array_equal(bits(t), bits(start[:3, 3]))
    R, t, it, err, why = ctx.icp_gicp_register(moving, cov_b, fixed, cov_a, capi.plane_params(max_iterations=0))
    assert it == 0 and np.array_equal(R, np.eye(3, dtype=np.float32)) and np.array_equal(t, np.zeros(3, np.float32))
    R, t, it, err, why = ctx.icp_gicp_register(moving, cov_b, fixed, cov_a, capi.plane_params(max_iterations=2, max_distance_squared=LIMIT))
    assert (it, why) == (2, capi.STOP_MAX_ITERATIONS)
    ref = reference_run("origin", K.DIST_CPU_ROUNDING, 2)
    assert np.abs(R - ref["R"]).max() <= 1e-6 and np.abs(t - ref["t"]).max() <= 1e-6


# ---- 4. one iteration from a given start
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", SCENES)
def test_one_iteration_from_the_restatements_poses(ctx, capi, name, mode):
    moving, cov_b, fixed, cov_a, _, _ = gscene(name)
    run = reference_run(name, mode)
    assert len(run["poses"]) >= 3
    c0 = np.abs(P.centre(fixed)).max()
    for k, pose in enumerate(run["poses"]):
        Tk = P.pose44(*pose)
        st = G.step(moving, cov_b, fixed, cov_a, Tk[:3, :3].astype(np.float64), Tk[:3, 3].astype(np.float64), mode, LIMIT)
        assert st["stop"] is None and st["kappa"] <= 1e4, (name, k, st["kappa"])
        R, t, it, err, why = ctx.icp_gicp_register(moving, cov_b, fixed, cov_a, capi.plane_params(max_iterations=1, max_distance_squared=LIMIT, dist_mode=mode,
                                                                                                  eps_rotation=0.0, eps_translation=0.0), init=Tk)
        assert it == 1 and why == capi.STOP_MAX_ITERATIONS
        got, want = np.concatenate([R.ravel(), t]).astype(np.float64), np.concatenate([st["R"].ravel(), st["t"]])
        bound = 2.0 ** -23 * np.maximum(1, np.abs(want)) + 1e-12 * st["kappa"] * max(1.0, c0)
        print("%s mode %d step %d: cond(S) %.2f, worst entry %.2e of its bound, error %.3e" % (name, mode, k, st["kappa"], (np.abs(got - want) / bound).max(), err))
        assert (np.abs(got - want) <= bound).all(), (name, k, np.abs(got - want), bound)
        assert abs(np.float64(err) - np.float64(st["error"])) <= np.spacing(np.float32(st["error"])), (name, k, err, st["error"])


# ---- 5. whole registrations
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", SCENES)
def test_whole_registration_reaches_the_ground_truth(ctx, capi, name, mode):
    moving, cov_b, fixed, cov_a, Gt, _ = gscene(name)
    run = reference_run(name, mode)
    assert run["stop"] == G.STOP_CONVERGED
    params = capi.plane_params(max_distance_squared=LIMIT, dist_mode=mode, eps_translation=EPS_TRANSLATION[name])
    R, t, it, err, why = ctx.icp_gicp_register(moving, cov_b, fixed, cov_a, params)
    assert why == capi.STOP_CONVERGED
    dR, dt = distance(R, t, Gt)
    rR, rt = distance(run["R"], run["t"], Gt)
    print("%s mode %d: device %d iterations, |dR| %.2e |dt| %.2e, error %.3e; restatement %d iterations, |dR| %.2e |dt| %.2e" % (
        name, mode, it, dR, dt, err, run["iterations"], rR, rt))
    assert dR <= 4 * rR + np.spacing(np.float32(1.0))
    assert dt <= 4 * rt + np.spacing(np.float32(np.abs(Gt[:3, 3]).max()))
    assert abs(it - run["iterations"]) <= 2
    # covariances estimated on the device in place of the analytic ones
    est_a, est_b = ctx.estimate_covariances(fixed, 16, capi.COV_PLANE, EPS, mode), ctx.estimate_covariances(moving, 16, capi.COV_PLANE, EPS, mode)
    R, t, ite, erre, why = ctx.icp_gicp_register(moving, est_b, fixed, est_a, params)
    eR, et = distance(R, t, Gt)
    print("%s mode %d: estimated covariances (k = 16) %d iterations, |dR| %.2e |dt| %.2e against the analytic %.2e %.2e" % (name, mode, ite, eR, et, dR, dt))
    assert why == capi.STOP_CONVERGED
    assert eR <= 10 * dR and et <= 10 * dt


# ---- 6. the contract
def test_same_bits_whatever_ran_before_and_whatever_the_batch(ctx, capi, bunny):
    moving, cov_b, fixed, cov_a, _, normals = gscene("origin")

    def run(**kw):
        R, t, it, err, why = ctx.icp_gicp_register(moving, cov_b, fixed, cov_a, capi.plane_params(max_distance_squared=LIMIT, **kw))
        return bits(R).tolist(), bits(t).tolist(), it, bits(np.float32(err)).tolist(), why

    first = run()
    assert run() == first
    ctx.knn_search(None, fixed, 8)
    ctx.icp_plane_register(moving, fixed, normals.astype(np.float32), capi.plane_params(max_distance_squared=LIMIT))
    ctx.cpd_register(bunny[0][:300], bunny[1][:300], capi.cpd_params(max_iterations=3))
    ctx.estimate_covariances(fixed[:500], 8)
    assert run() == first
    for sync_every in (1, 4, 7):
        assert run(sync_every=sync_every) == first
    ctx.profile_enable(True)
    try:
        assert run() == first
        times = ctx.icp_gicp_times()
    finally:
        ctx.profile_enable(False)
    assert times["total"] > 0 and times["iterations"] > 0 and all(v >= 0 for v in times.values())


def test_a_loaded_icp_problem_survives(ctx, capi, bunny):
    before, after = bunny
    moving, cov_b, fixed, cov_a, _, _ = gscene("origin")
    params = capi.icp_params(eps=1e-9, max_iterations=12)

    def icp(between):
        ctx.icp_load(before, after, params)
        ctx.icp_run(5)
        if between:
            ctx.icp_gicp_register(moving, cov_b, fixed, cov_a, capi.plane_params(max_distance_squared=LIMIT))
            ctx.gicp_system(moving, cov_b, fixed, cov_a)
            ctx.estimate_covariances(fixed, 8)
        ctx.icp_run(7)
        R, t, it, err, why = ctx.icp_result()
        return bits(R).tolist(), bits(t).tolist(), it, bits(np.float32(err)).tolist(), why

    assert icp(True) == icp(False)


def test_no_buffer_outlives_its_context(capi, ctx):
    """(the session's context keeps its own buffers: the count goes back to where it was, 0 of this context's left)"""
    moving, cov_b, fixed, cov_a, _, _ = gscene("origin")
    start = capi.selftest_live_buffers()
    with capi.Context(0) as own:
        own.profile_enable(True)
        own.icp_gicp_register(moving, cov_b, fixed, cov_a, capi.plane_params(max_distance_squared=LIMIT))
        own.gicp_system(moving, cov_b, fixed, cov_a)
        own.estimate_covariances(fixed, 8, want_count=True)
        assert capi.selftest_live_buffers() > start
    assert capi.selftest_live_buffers() - start == 0


# ---- 7. refusals: nothing is written
def test_invalid_arguments_are_refused_with_the_outputs_untouched(ctx, capi):
    moving, cov_b, fixed, cov_a, _, _ = gscene("origin")
    moving, cov_b, fixed, cov_a = moving[:200].copy(), cov_b[:200].copy(), fixed[:300].copy(), cov_a[:300].copy()
    n, m = len(moving), len(fixed)
    nan, inf = float("nan"), float("inf")

    def spoiled(a, row, value, col=1):
        a = a.copy()
        a[row, col] = value
        return a

    def register(what, before=moving, cb=cov_b, after=fixed, ca=cov_a, n=n, m=m, init=None, null=(), **kw):
        p = capi.plane_params(**kw)
        T, it, err, why = np.full(16, -7.5, np.float32), C.c_int(-7), C.c_float(-7.5), C.c_int(-7)
        ptr = {"before": before.ctypes.data, "before_cov": cb.ctypes.data, "after": after.ctypes.data, "after_cov": ca.ctypes.data, "params": C.addressof(p),
               "out_T": T.ctypes.data}
        for k in null:
            ptr[k] = None
        rc = capi.icp_gicp_register_raw(ctx._h, ptr["before"], ptr["before_cov"], n, ptr["after"], ptr["after_cov"], m, ptr["params"],
                                        None if init is None else init.ctypes.data, ptr["out_T"], C.addressof(it), C.addressof(err), C.addressof(why))
        msg = capi.lib().mi_last_error().decode()
        assert rc == capi.MI_ERR_INVALID_ARG and msg.startswith("mi_icp_gicp_register"), (what, rc, msg)
        assert (T == -7.5).all() and it.value == -7 and err.value == -7.5 and why.value == -7, what
        return msg

    for k in ("before", "before_cov", "after", "after_cov", "params", "out_T"):
        register("null " + k, null=(k,))
    register("n = 0", n=0)
    register("m = 0", m=0)
    register("dist_mode", dist_mode=2)
    register("limit nan", max_distance_squared=nan)
    register("limit negative", max_distance_squared=-1.0)
    register("eps_rotation negative", eps_rotation=-1e-3)
    register("eps_translation nan", eps_translation=nan)
    register("max_iterations", max_iterations=-1)
    register("sync_every", sync_every=-1)
    assert "before_xyz point 17" in register("before nan", before=spoiled(spoiled(moving, 17, nan), 150, nan))
    assert "after_xyz point 5" in register("after inf", after=spoiled(fixed, 5, inf))
    assert "after_xyz point 6" in register("after large", after=spoiled(fixed, 6, 2e18))
    assert "before_cov6 covariance 11 " in register("moving covariance nan", cb=spoiled(spoiled(cov_b, 11, nan, 5), 120, nan, 0))
    assert "before_cov6 covariance 12 " in register("moving covariance large", cb=spoiled(cov_b, 12, -2e18, 3))
    assert "after_cov6 covariance 9 " in register("fixed covariance inf", ca=spoiled(spoiled(cov_a, 9, inf, 4), 299, nan, 2))
    assert "after_cov6 covariance 0 " in register("fixed covariance -inf", ca=spoiled(cov_a, 0, -inf, 0))
    bad = np.eye(4, dtype=np.float32).reshape(16)
    bad[13] = inf
    assert "entry 13" in register("transform", init=bad)

    def system(what, before=moving, cb=cov_b, ca=cov_a, T=None, mode=0, max_d2=inf, n=n, null_sums=False):
        sums, centre, idx = np.full(32, -7.5), np.full(3, -7.5, np.float32), np.full(len(before), -7, np.int32)
        rc = capi.gicp_system_raw(ctx._h, before.ctypes.data, cb.ctypes.data, n, fixed.ctypes.data, ca.ctypes.data, m, None if T is None else T.ctypes.data, mode,
                                  max_d2, None if null_sums else sums.ctypes.data, centre.ctypes.data, idx.ctypes.data)
        msg = capi.lib().mi_last_error().decode()
        assert rc == capi.MI_ERR_INVALID_ARG and msg.startswith("mi_gicp_system"), (what, rc, msg)
        assert (sums == -7.5).all() and (centre == -7.5).all() and (idx == -7).all(), what
        return msg

    system("n = 0", n=0)
    system("null sums", null_sums=True)
    system("dist_mode", mode=7)
    system("limit", max_d2=-0.5)
    system("before nan", before=spoiled(moving, 3, nan))
    assert "before_cov6 covariance 3 " in system("covariance nan", cb=spoiled(cov_b, 3, nan))
    assert "after_cov6 covariance 7 " in system("covariance large", ca=spoiled(cov_a, 7, 1.5e18))
    system("transform", T=bad)
    # the largest covariance entries the call accepts, and the context still works
    ctx.gicp_system(moving, spoiled(cov_b, 3, 1e18), fixed, cov_a)
    loose = np.eye(4, dtype=np.float32)
    loose[3] = nan                                         # the bottom row of a transform is never read
    assert np.array_equal(bits(ctx.gicp_system(moving, cov_b, fixed, cov_a, loose)[0]), bits(ctx.gicp_system(moving, cov_b, fixed, cov_a)[0]))
    assert ctx.gicp_system(moving, cov_b, fixed, cov_a)[0][29] > 0
