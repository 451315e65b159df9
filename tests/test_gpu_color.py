"""GPU suite of mi_estimate_color_gradients, mi_icp_color_register and mi_color_system against the float64 restatement of
tests/color_reference.py.  The restatement's O(n m) parts, the keys of tests/knn_reference.py, are worked once per scene, pose and mode
(lru_cache) and shared.

The scenes (color_reference.scene): 4 000 fixed points, x and y uniform in [-2, 2], on z = 0.3 sin(1.5 x) cos(1.2 y) ("wave") or on
z = 0 exactly with normals (0, 0, 1) ("flat"), with I = 0.5 + 0.2 sin(2 x) + 0.2 cos(1.7 y) in fp32; the moving cloud is 3 000 of them
under the inverse of the ground truth G.  "shifted" is "wave" moved by (100, -50, 25) and runs with eps_translation = 1e-4, as in
tests/test_gpu_plane.py.  The registrations take the RESTATEMENT's gradients (k = 16), so that they do not lean on K48.

The bounds (none of them taken from what the device gives):
  gradients    count equal to mi_knn_search's; zeros exactly where the rule says; elsewhere per component
               |delta| <= 2^-23 |d|_inf + 64 2^-53 cond_1(M) |d|_inf against the restatement's unrounded d: one fp32 unit for the output
               rounding plus the 3 x 3 solve's backward error.  Points with cond_1(M) > 1e8 are left out, at most 1 % of a case
               (tests/test_color_reference.py holds the scene to that)
  sums         idx, the centre and the pair count equal; every other sum within (n + 8) 2^-53 sum |term|, as tests/test_gpu_plane.py
               derives it; at lambda = 1 equal to mi_plane_system's
  one step     every entry of out_T within 2^-23 max(1, |entry|) + 1e-12 cond(S) max(1, |c0|) of the restatement's step from the same
               fp32 pose, cond(S) <= 1e3 asserted
  whole runs   max |dR| and max |dt| from the ground truth at most 4 x the restatement's own plus one fp32 unit of the largest entry"""
import ctypes as C
import functools

import numpy as np
import pytest

import color_reference as CR
import knn_reference as K
import plane_reference as P

pytestmark = pytest.mark.gpu

MODES = (K.DIST_CPU_ROUNDING, K.DIST_FMA)
LIMIT = 0.25
LAMBDAS = (0.0, CR.LAMBDA, 1.0)
EPS_TRANSLATION = {"wave": 1e-6, "flat": 1e-6, "shifted": 1e-4}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


@functools.lru_cache(maxsize=None)
def scene(name):
    """color_reference.scene(name) with the restatement's gradients of the fixed cloud from 16 neighbours"""
    s = dict(CR.scene(name))
    s["grad"] = CR.frozen(CR.gradients(s["fixed"], s["normals"], s["ia"], 16)["grad"])
    return s


def fixed_of(s):
    return s["fixed"], s["normals"], s["ia"], s["grad"]


# ---- 1. gradients
def check_gradients(ctx, cloud, normals, intensity, k, mode, limit, what, only=None):
    grad, count = ctx.estimate_color_gradients(cloud, normals, intensity, k, mode, limit, want_count=True)
    _, kcount = ctx.knn_search(None, cloud, k, mode, limit, want_d2=False, want_count=True)
    assert np.array_equal(count, kcount), what
    ref = CR.gradients(cloud, normals, intensity, k, mode, limit, only=only)
    rows = np.arange(len(cloud)) if only is None else np.asarray(only)
    got = grad[rows]
    assert np.array_equal(count[rows], ref["count"]), what
    assert (got[~ref["solved"]] == 0).all(), what
    cond = np.full(len(rows), np.inf)
    cond[ref["solved"]] = CR.cond1(ref["M"][ref["solved"]])
    well = ref["solved"] & (cond <= CR.ILL_CONDITIONED)
    left_out = int((ref["solved"] & ~well).sum())
    assert left_out <= CR.ILL_SHARE * len(rows), (what, left_out)
    dinf = np.abs(ref["d"]).max(axis=1)
    bound = 2.0 ** -23 * dinf + 64 * 2.0 ** -53 * np.where(well, cond, 0.0) * dinf
    err = np.abs(got.astype(np.float64) - ref["d"])
    equal = float((bits(got) == bits(ref["grad"])).all(axis=1).mean())
    shown = well & (bound > 0)
    worst = (err[shown].max(axis=1) / bound[shown]).max(initial=0.0)
    print("%s: %d rows, %d solved, %d left out; bit-equal share %.4f; worst error %.2e of its bound" % (what, len(rows), ref["solved"].sum(), left_out, equal, worst))
    assert np.isfinite(got).all() and (err[well] <= bound[well, None]).all(), what
    return grad, count, ref


@pytest.mark.parametrize("n", [1, 3, 64, 65])
def test_gradients_small_clouds(ctx, n):
    g = CR.gradient_scene("wave")
    for k in CR.GRADIENT_KS:
        for mode in MODES:
            check_gradients(ctx, g["cloud"][:n], g["normals"][:n], g["intensity"][:n], k, mode, np.inf, "wave n %d k %d mode %d" % (n, k, mode))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["wave", "flat"])
def test_gradients_of_the_scene_and_the_planted_zeros(ctx, name, mode):
    g = CR.gradient_scene(name)
    for k in CR.GRADIENT_KS:
        grad, count, ref = check_gradients(ctx, g["cloud"], g["normals"], g["intensity"], k, mode, CR.GRADIENT_LIMIT, "%s k %d mode %d" % (name, k, mode))
        assert (grad[g["zero"]] == 0).all() and (count[g["zero"]] == k).all()                 # a zero normal
        assert (grad[g["line"]] == 0).all() and (count[g["line"]] == min(k, 3)).all()         # collinear neighbours: det = 0 exactly
        assert (grad[g["lonely"]] == 0).all() and count[g["lonely"]] == 0                     # no neighbour within the limit
        assert ref["solved"].sum() >= 3900 and (np.abs(grad[:4000]).max(axis=1) > 0).sum() >= 3900
    if name == "flat":          # the analytic gradient of the texture, to the least squares' truncation at k = 32's radius
        x, y = g["cloud"][:4000, 0].astype(np.float64), g["cloud"][:4000, 1].astype(np.float64)
        inner = (np.abs(x) < 1.6) & (np.abs(y) < 1.6) & (np.abs(grad[:4000]).max(axis=1) > 0)
        want = np.stack([0.4 * np.cos(2 * x), -0.34 * np.sin(1.7 * y), np.zeros(4000)], axis=1)
        assert np.abs(grad[:4000][inner] - want[inner]).max() <= 0.1


@pytest.mark.parametrize("mode", MODES)
def test_gradients_beyond_one_grid_shape(ctx, mode):
    """50 000 jittered copies of the wave's points: another grid than the scene's; the restatement on 300 rows, the counts on all"""
    s = CR.scene("wave")
    rng = np.random.default_rng(5)
    src = rng.integers(0, 4000, 50000)
    cloud = (s["fixed"][src] + rng.normal(0, 0.01, (50000, 3))).astype(np.float32)
    only = np.sort(rng.permutation(50000)[:300])
    check_gradients(ctx, cloud, s["normals"][src], CR.texture(cloud[:, :2].astype(np.float64)), 16, mode, np.inf, "50000 points mode %d" % mode, only=only)


# ---- 2. one linearisation
def pose_of(T):
    return (np.eye(3), np.zeros(3)) if T is None else (np.asarray(T, np.float64)[:3, :3], np.asarray(T, np.float64)[:3, 3])


def moving_of(s, n):
    """the scene's first n moving points and intensities; beyond its 3 000, copies of them 1e-3 off"""
    moving, ib = s["moving"], s["ib"]
    if n <= len(moving):
        return moving[:n], ib[:n]
    rng = np.random.default_rng(5)
    pick = rng.integers(0, len(moving), n - len(moving))
    return np.concatenate([moving, (moving[pick] + rng.normal(0, 1e-3, (len(pick), 3))).astype(np.float32)]), np.concatenate([ib, ib[pick]])


def check_system(ctx, moving, ib, s, T, mode, lam, what, keys=None):
    """keys: the restatement's matches of an earlier call at the same pose and mode (they do not depend on lambda); kept in check_system.keys"""
    R, t = pose_of(T)
    ref = CR.system(moving, ib, *fixed_of(s), R, t, mode, LIMIT, lam, keys=keys)
    check_system.keys = ref["keys"]
    sums, centre, idx = ctx.color_system(moving, ib, *fixed_of(s), T, mode, LIMIT, lam)
    assert np.array_equal(idx, ref["idx"]), what
    assert np.array_equal(bits(centre), bits(ref["centre"])), what
    assert sums[29] == ref["sums"][29] and (sums[30:] == 0).all(), what
    bound = (len(moving) + 8) * 2.0 ** -53 * ref["abs"][:29]
    err = np.abs(sums[:29] - ref["sums"][:29])
    print("%s: %d pairs; worst sum error %.2e of its bound" % (what, int(sums[29]), (err[bound > 0] / bound[bound > 0]).max(initial=0.0)))
    assert (err <= bound).all(), (what, err, bound)
    if lam == 1.0:
        plane = ctx.plane_system(moving, s["fixed"], s["normals"], T, mode, LIMIT)
        assert (sums == plane[0]).all() and np.array_equal(idx, plane[2]), what
    return sums


@pytest.mark.parametrize("name", ["wave", "flat"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 3000, 4097])
def test_color_system_sizes(ctx, n, name):
    s = scene(name)
    moving, ib = moving_of(s, n)
    for mode in MODES:
        for label, T in (("null", None), ("truth", s["G"].astype(np.float32))):
            keys = None
            for lam in LAMBDAS:
                sums = check_system(ctx, moving, ib, s, T, mode, lam, "%s n %d mode %d T %s lambda %g" % (name, n, mode, label, lam), keys)
                keys = check_system.keys
    assert sums[29] == n


@pytest.mark.parametrize("mode", MODES)
def test_color_system_beyond_the_rows_one_workgroup_sums(ctx, mode):
    """70 000 moving points are 1 094 rows: the slabs come first (three launches).  The device's matches are held to mi_knn_search's, bit
    for bit, and all 29 sums to the restatement's float64 terms of those pairs."""
    s = scene("wave")
    rng = np.random.default_rng(5)
    pick = rng.integers(0, 4000, 70000)
    big, ib = (s["fixed"][pick] + rng.normal(0, 1e-3, (70000, 3))).astype(np.float32), s["ia"][pick]
    sums, centre, idx = ctx.color_system(big, ib, *fixed_of(s), None, mode, LIMIT, CR.LAMBDA)
    again = ctx.color_system(big, ib, *fixed_of(s), None, mode, LIMIT, CR.LAMBDA)
    assert np.array_equal(bits(sums), bits(again[0])) and np.array_equal(idx, again[2])
    kidx, kd2 = ctx.knn_search(big, s["fixed"], 1, mode, LIMIT)
    assert np.array_equal(idx, kidx[:, 0]) and sums[29] == 70000 and (sums[30:] == 0).all()
    want, mags = CR.sums_of_pairs(P.move_f32(np.eye(3), np.zeros(3), big), ib, *fixed_of(s), idx, kd2[:, 0], CR.LAMBDA)
    bound = (70000 + 8) * 2.0 ** -53 * mags[:29]
    err = np.abs(sums[:29] - want[:29])
    print("70000 points mode %d: worst sum error %.2e of its bound" % (mode, (err / bound).max()))
    assert (err <= bound).all(), (err, bound)


def test_a_zero_gradient_is_still_a_pair_and_a_zero_normal_is_none(ctx):
    s = scene("wave")
    holes = dict(s)
    rng = np.random.default_rng(7)
    grad, normals = s["grad"].copy(), s["normals"].copy()
    grad[rng.permutation(4000)[:400]] = 0
    normals[rng.permutation(4000)[:200]] = 0
    holes["grad"], holes["normals"] = grad, normals
    sums = check_system(ctx, s["moving"], s["ib"], holes, s["G"].astype(np.float32), K.DIST_CPU_ROUNDING, CR.LAMBDA, "holes")
    assert 2700 <= sums[29] < 3000


# ---- 3. one step and 4. whole runs
@functools.lru_cache(maxsize=None)
def reference_run(name, mode):
    s = scene(name)
    return CR.register(s["moving"], s["ib"], *fixed_of(s), 1e-6, EPS_TRANSLATION[name], 50, LIMIT, mode, CR.LAMBDA)


def register(ctx, capi, s, lam=CR.LAMBDA, init=None, **kw):
    return ctx.icp_color_register(s["moving"], s["ib"], *fixed_of(s), capi.plane_params(max_distance_squared=LIMIT, **kw), lam, init)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["wave", "flat", "shifted"])
def test_one_iteration_from_the_restatements_poses(ctx, capi, name, mode):
    s = scene(name)
    run = reference_run(name, mode)
    assert len(run["poses"]) >= 3
    c0 = np.abs(P.centre(s["fixed"])).max()
    for k in range(3):
        Tk = P.pose44(*run["poses"][k])
        st = CR.step(s["moving"], s["ib"], *fixed_of(s), Tk[:3, :3].astype(np.float64), Tk[:3, 3].astype(np.float64), mode, LIMIT, CR.LAMBDA)
        assert st["stop"] is None and st["kappa"] <= 1e3, (name, k, st["kappa"])
        R, t, it, err, why = register(ctx, capi, s, init=Tk, max_iterations=1, dist_mode=mode, eps_rotation=0.0, eps_translation=0.0)
        assert it == 1 and why == capi.STOP_MAX_ITERATIONS
        got, want = np.concatenate([R.ravel(), t]).astype(np.float64), np.concatenate([st["R"].ravel(), st["t"]])
        bound = 2.0 ** -23 * np.maximum(1, np.abs(want)) + 1e-12 * st["kappa"] * max(1.0, c0)
        print("%s mode %d step %d: cond(S) %.2f, worst entry %.2e of its bound, error %.3e" % (name, mode, k, st["kappa"], (np.abs(got - want) / bound).max(), err))
        assert (np.abs(got - want) <= bound).all(), (name, k, np.abs(got - want), bound)
        assert abs(np.float64(err) - np.float64(st["error"])) <= np.spacing(np.float32(st["error"])), (name, k, err, st["error"])


def distance(R, t, G):
    return np.abs(np.asarray(R, np.float64) - G[:3, :3]).max(), np.abs(np.asarray(t, np.float64) - G[:3, 3]).max()


def test_plane_icp_is_degenerate_on_the_flat_scene(ctx, capi):
    s = scene("flat")
    start = P.pose44(P.rodrigues([0.0, 0.0, 0.01]), [0.01, 0.0, 0.0])
    R, t, it, err, why = ctx.icp_plane_register(s["moving"], s["fixed"], s["normals"], capi.plane_params(max_distance_squared=LIMIT), init=start)
    assert (it, why) == (0, capi.STOP_DEGENERATE) and np.array_equal(bits(R), bits(start[:3, :3])) and np.array_equal(bits(t), bits(start[:3, 3]))
    R, t, it, err, why = register(ctx, capi, s, lam=1.0, init=start)
    assert (it, why) == (0, capi.STOP_DEGENERATE) and np.array_equal(bits(R), bits(start[:3, :3])) and np.array_equal(bits(t), bits(start[:3, 3]))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["flat", "wave", "shifted"])
def test_whole_registration_reaches_the_ground_truth(ctx, capi, name, mode):
    s = scene(name)
    G = s["G"]
    run = reference_run(name, mode)
    assert run["stop"] == P.STOP_CONVERGED
    R, t, it, err, why = register(ctx, capi, s, dist_mode=mode, eps_translation=EPS_TRANSLATION[name])
    assert why == capi.STOP_CONVERGED
    dR, dt = distance(R, t, G)
    rR, rt = distance(run["R"], run["t"], G)
    print("%s mode %d: device %d iterations, |dR| %.2e |dt| %.2e, error %.3e; restatement %d iterations, |dR| %.2e |dt| %.2e" % (
        name, mode, it, dR, dt, err, run["iterations"], rR, rt))
    assert dR <= 4 * rR + np.spacing(np.float32(1.0))
    assert dt <= 4 * rt + np.spacing(np.float32(np.abs(G[:3, 3]).max()))


def test_same_bits_whatever_ran_before_and_whatever_the_batch(ctx, capi):
    s = scene("flat")

    def run(**kw):
        R, t, it, err, why = register(ctx, capi, s, **kw)
        return bits(R).tolist(), bits(t).tolist(), it, bits(np.float32(err)).tolist(), why

    first = run()
    assert first[4] == capi.STOP_CONVERGED and run() == first
    ctx.knn_search(None, s["fixed"], 8)
    ctx.estimate_normals(s["fixed"], 8)
    ctx.estimate_color_gradients(s["fixed"], s["normals"], s["ia"], 8)
    ctx.icp_plane_register(s["moving"], s["fixed"], s["normals"], capi.plane_params(max_distance_squared=LIMIT))
    assert run() == first
    for sync_every in (1, 4, 50):
        assert run(sync_every=sync_every) == first
    ctx.profile_enable(True)
    try:
        assert run() == first
        times = ctx.icp_color_times()
    finally:
        ctx.profile_enable(False)
    assert times["total"] > 0 and times["iterations"] > 0 and all(v >= 0 for v in times.values())
    R, t, it, err, why = register(ctx, capi, s, max_iterations=0)
    assert (it, err, why) == (0, 0.0, capi.STOP_MAX_ITERATIONS) and np.array_equal(R, np.eye(3, dtype=np.float32)) and (t == 0).all()


def test_the_device_gradients_register_the_flat_scene_too(ctx, capi):
    """the pipeline as a caller runs it: K48's gradients into K49's loop"""
    s = dict(scene("flat"))
    s["grad"] = ctx.estimate_color_gradients(s["fixed"], s["normals"], s["ia"], 16)
    R, t, it, err, why = register(ctx, capi, s)
    dR, dt = distance(R, t, s["G"])
    assert why == capi.STOP_CONVERGED and dR <= 1e-4 and dt <= 1e-4, (why, it, dR, dt)


# ---- 5. refusals and state
def test_invalid_arguments_are_refused_with_the_outputs_untouched(ctx, capi):
    s = scene("wave")
    moving, ib = s["moving"][:200].copy(), s["ib"][:200].copy()
    fixed, normals, ia, grad = (a[:300].copy() for a in fixed_of(s))
    n, m = len(moving), len(fixed)
    nan, inf = float("nan"), float("inf")

    def spoiled(a, row, value):
        a = a.copy()
        if a.ndim == 2:
            a[row, 1] = value
        else:
            a[row] = value
        return a

    arrays = dict(before=moving, ib=ib, after=fixed, normals=normals, ia=ia, grad=grad)

    def register(what, n=n, m=m, lam=0.968, init=None, null=(), params=True, **kw):
        use = dict(arrays, **{k: kw.pop(k) for k in list(kw) if k in arrays})
        p = capi.plane_params(**kw)
        T, it, err, why = np.full(16, -7.5, np.float32), C.c_int(-7), C.c_float(-7.5), C.c_int(-7)
        ptr = {k: v.ctypes.data for k, v in use.items()}
        ptr.update(params=C.addressof(p), out_T=T.ctypes.data)
        for k in null:
            ptr[k] = None
        rc = capi.icp_color_register_raw(ctx._h, ptr["before"], ptr["ib"], n, ptr["after"], ptr["normals"], ptr["ia"], ptr["grad"], m, ptr["params"], lam,
                                         None if init is None else init.ctypes.data, ptr["out_T"], C.addressof(it), C.addressof(err), C.addressof(why))
        msg = capi.lib().mi_last_error().decode()
        assert rc == capi.MI_ERR_INVALID_ARG and msg.startswith("mi_icp_color_register"), (what, rc, msg)
        assert (T == -7.5).all() and it.value == -7 and err.value == -7.5 and why.value == -7, what
        return msg

    for k in ("before", "ib", "after", "normals", "ia", "grad", "params", "out_T"):
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
    for lam in (nan, -0.01, 1.01, inf):
        assert "lambda_geometric" in register("lambda %r" % lam, lam=lam)
    assert "before_xyz point 17" in register("before nan", before=spoiled(moving, 17, nan))
    assert "after_xyz point 5" in register("after inf", after=spoiled(fixed, 5, inf))
    assert "after_xyz point 6" in register("after large", after=spoiled(fixed, 6, 2e18))
    assert "after_normals_xyz normal 9" in register("normal nan", normals=spoiled(normals, 9, nan))
    assert "before_intensity value 11" in register("ib nan", ib=spoiled(spoiled(ib, 150, inf), 11, nan))
    assert "after_intensity value 7" in register("ia large", ia=spoiled(spoiled(ia, 7, -2e18), 250, nan))
    assert "after_gradients_xyz gradient 3" in register("grad inf", grad=spoiled(spoiled(grad, 3, -inf), 299, nan))
    bad = np.eye(4, dtype=np.float32).reshape(16)
    bad[13] = inf
    assert "entry 13" in register("transform", init=bad)

    def system(what, T=None, mode=0, max_d2=inf, lam=0.968, n=n, **kw):
        use = dict(arrays, **kw)
        sums, centre, idx = np.full(32, -7.5), np.full(3, -7.5, np.float32), np.full(len(moving), -7, np.int32)
        rc = capi.color_system_raw(ctx._h, use["before"].ctypes.data, use["ib"].ctypes.data, n, use["after"].ctypes.data, use["normals"].ctypes.data,
                                   use["ia"].ctypes.data, use["grad"].ctypes.data, m, None if T is None else T.ctypes.data, mode, max_d2, lam,
                                   sums.ctypes.data, centre.ctypes.data, idx.ctypes.data)
        msg = capi.lib().mi_last_error().decode()
        assert rc == capi.MI_ERR_INVALID_ARG and msg.startswith("mi_color_system"), (what, rc, msg)
        assert (sums == -7.5).all() and (centre == -7.5).all() and (idx == -7).all(), what
        return msg

    system("n = 0", n=0)
    system("dist_mode", mode=7)
    system("limit", max_d2=-0.5)
    system("lambda", lam=1.5)
    system("transform", T=bad)
    assert "before_xyz point 3" in system("before nan", before=spoiled(moving, 3, nan))
    assert "after_gradients_xyz gradient 8" in system("grad nan", grad=spoiled(grad, 8, nan))
    assert "before_intensity value 0" in system("ib inf", ib=spoiled(ib, 0, inf))

    def gradients(what, cloud=fixed, nrm=normals, I=ia, n=m, k=8, mode=0, max_d2=inf, null=()):
        out, count = np.full((m, 3), -7.5, np.float32), np.full(m, -7, np.int32)
        ptr = dict(cloud=cloud.ctypes.data, nrm=nrm.ctypes.data, I=I.ctypes.data, out=out.ctypes.data)
        for key in null:
            ptr[key] = None
        rc = capi.estimate_color_gradients_raw(ctx._h, ptr["cloud"], ptr["nrm"], ptr["I"], n, k, mode, max_d2, ptr["out"], count.ctypes.data)
        msg = capi.lib().mi_last_error().decode()
        assert rc == capi.MI_ERR_INVALID_ARG and msg.startswith("mi_estimate_color_gradients"), (what, rc, msg)
        assert (out == -7.5).all() and (count == -7).all(), what
        return msg

    for key in ("cloud", "nrm", "I", "out"):
        gradients("null " + key, null=(key,))
    gradients("n = 0", n=0)
    gradients("k = 1", k=1)
    gradients("k = 33", k=33)
    gradients("dist_mode", mode=3)
    gradients("limit", max_d2=nan)
    assert "cloud_xyz point 4" in gradients("cloud nan", cloud=spoiled(fixed, 4, nan))
    assert "normals_xyz normal 2" in gradients("normal inf", nrm=spoiled(normals, 2, inf))
    assert "intensity value 12" in gradients("intensity", I=spoiled(spoiled(ia, 12, nan), 200, inf))
    # the context still works
    assert ctx.color_system(moving, ib, fixed, normals, ia, grad)[0][29] > 0


def test_a_loaded_icp_problem_survives(ctx, capi, bunny):
    before, after = bunny
    s = scene("wave")
    params = capi.icp_params(eps=1e-9, max_iterations=12)

    def icp(between):
        ctx.icp_load(before, after, params)
        ctx.icp_run(5)
        if between:
            register(ctx, capi, s)
            ctx.color_system(s["moving"], s["ib"], *fixed_of(s))
            ctx.estimate_color_gradients(s["fixed"], s["normals"], s["ia"], 8)
        ctx.icp_run(7)
        R, t, it, err, why = ctx.icp_result()
        return bits(R).tolist(), bits(t).tolist(), it, bits(np.float32(err)).tolist(), why

    assert icp(True) == icp(False)


def test_no_buffer_outlives_its_context(capi, ctx):
    """(the session's context keeps its own buffers: the count goes back to where it was, 0 of this context's left)"""
    s = scene("wave")
    start = capi.selftest_live_buffers()
    with capi.Context(0) as own:
        own.profile_enable(True)
        register(own, capi, s)
        own.color_system(s["moving"], s["ib"], *fixed_of(s))
        own.estimate_color_gradients(s["fixed"], s["normals"], s["ia"], 8)
        assert capi.selftest_live_buffers() > start
    assert capi.selftest_live_buffers() - start == 0
