"""GPU suite of mi_evaluate_registration against the float64 restatement of tests/eval_reference.py.

The scene is the plane suite's (tests/test_gpu_plane.py), restated here: 4 000 fixed points on z = 0.3 sin(1.5 x) cos(1.2 y), x and y uniform
in [-2, 2]; the moving cloud is 3 000 of them moved by the inverse of G, a rotation of 5 degrees about (1, 2, 3) through the centroid and a
translation of (0.05, -0.03, 0.04), so that G is the ground truth.  "shifted" is the same scene moved by (100, -50, 25).  Three poses: NULL
(the clouds 5 degrees apart), G, and G with 0.3 more along x -- along the surface, so that under the limit 0.25^2 the points near the +x
edge lose their partner and the rest keep one: 0 < fitness < 1, asserted of the restatement.

The bounds (none of them taken from what the device gives):
  pairs        idx, the bits of d2 and the pair count equal the restatement's
  sums         every sum in [0, 29) within (n + 8) 2^-53 sum |term|, sum |term| formed by the restatement: the terms are the same float64
               operations on both sides, so what differs is the order of n additions (the plane suite's bound)
  the rest     fitness, RMSE and the information matrix are exactly the stated expressions of the device's own sums"""
import ctypes as C
import functools

import numpy as np
import pytest

import eval_reference as E
import knn_reference as K
import plane_reference as P

pytestmark = pytest.mark.gpu

MODES = (K.DIST_CPU_ROUNDING, K.DIST_FMA)
SCENES = ("origin", "shifted")
LIMIT = 0.25
POSES = ("null", "truth", "off")
POSE_LIMIT = {"null": LIMIT, "truth": LIMIT, "off": LIMIT * LIMIT}


def frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def scene(name):
    """(moving [3000, 3], fixed [4000, 3], unit normals [4000, 3], all float32; the ground truth G as a float64 [4, 4])"""
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


def pose(name, which):
    """the float32 [4, 4] transform of a pose's name, or None"""
    G = scene(name)[3]
    if which == "null":
        return None
    T = G.copy()
    if which == "off":
        T[:3, 3] += np.array([0.3, 0.0, 0.0])
    return T.astype(np.float32)


def pose_of(T):
    return (np.eye(3), np.zeros(3)) if T is None else (np.asarray(T, np.float64)[:3, :3], np.asarray(T, np.float64)[:3, 3])


def moving_of(name, n):
    """the scene's first n moving points; beyond its 3 000, copies of them 1e-3 off"""
    moving = scene(name)[0]
    if n <= len(moving):
        return moving[:n]
    rng = np.random.default_rng(5)
    extra = n - len(moving)
    return np.concatenate([moving, (moving[rng.integers(0, len(moving), extra)] + rng.normal(0, 1e-3, (extra, 3))).astype(np.float32)])


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def run(ctx, moving, fixed, T=None, pairs=None, mode=K.DIST_CPU_ROUNDING, max_d2=np.inf):
    """every output of one call: (fitness, rmse, sums, information, idx, d2)"""
    return ctx.evaluate_registration(moving, fixed, T, pairs, mode, max_d2, want_sums=True, want_information=True, want_idx=True, want_d2=True)


def same_outputs(a, b):
    return a[0] == b[0] and a[1] == b[1] and all(np.array_equal(bits(x), bits(y)) for x, y in zip(a[2:], b[2:]))


def check_derived(out, n, what):
    """fitness, RMSE and the information matrix are the stated float64 expressions of the call's own sums"""
    fitness, rmse, sums, info = out[:4]
    want_fitness, want_rmse = E.fitness_rmse(sums, n)
    assert bits(np.float64(fitness)) == bits(want_fitness) and bits(np.float64(rmse)) == bits(want_rmse), (what, fitness, rmse)
    assert np.array_equal(bits(info), bits(E.information(sums))) and np.array_equal(bits(info), bits(info.T)), what
    assert (sums[30:] == 0).all(), what


def check_sums(sums, want, mags, n, what):
    bound = (n + 8) * 2.0 ** -53 * mags[:29]
    err = np.abs(sums[:29] - want[:29])
    print("%s: %d pairs; worst sum error %.2e of its bound" % (what, int(sums[29]), (err[bound > 0] / bound[bound > 0]).max(initial=0.0)))
    assert sums[29] == want[29], what
    assert (err <= bound).all(), (what, err, bound)


def check(ctx, moving, fixed, T, mode, max_d2, what, pairs=None):
    """Test 1's comparison of one call against the restatement; returns (the device's answer, the restatement's)"""
    R, t = pose_of(T)
    ref = E.evaluate(moving, fixed, R, t, pairs, mode, max_d2)
    out = run(ctx, moving, fixed, T, pairs, mode, max_d2)
    fitness, rmse, sums, info, idx, d2 = out
    print("%s: fitness %.6f (restatement %.6f), RMSE %.6e (restatement %.6e)" % (what, fitness, ref["fitness"], rmse, ref["rmse"]))
    assert np.array_equal(idx, ref["idx"]), what
    assert np.array_equal(bits(d2), bits(ref["d2"])), what
    check_sums(sums, ref["sums"], ref["abs"], len(moving), what)
    check_derived(out, len(moving), what)
    return out, ref


# ---- 1. sizes, modes, scenes and poses against the restatement, element by element
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 3000, 4097])
def test_sizes_against_the_restatement(ctx, n, name, mode):
    fixed = scene(name)[1]
    for which in POSES:
        out, ref = check(ctx, moving_of(name, n), fixed, pose(name, which), mode, POSE_LIMIT[which], "%s n %d mode %d T %s" % (name, n, mode, which))
        if which == "off" and n > 1:           # (one point alone has a partner or has none)
            assert 0 < ref["fitness"] < 1, (name, n, ref["fitness"])


# ---- 2. beyond the rows one workgroup sums
@pytest.mark.parametrize("mode", MODES)
def test_beyond_the_rows_one_workgroup_sums(ctx, mode):
    """70 000 moving points are 1 094 rows, beyond PLANE_ONE_STAGE_ROWS: the slabs come first.  A restatement of the matches would cost n m
    here, so the device's matches are held to mi_knn_search's, bit for bit, and the sums to the restatement's float64 terms of those pairs,
    under the bound of every other case."""
    fixed = scene("origin")[1]
    rng = np.random.default_rng(5)
    big = (fixed[rng.integers(0, 4000, 70000)] + rng.normal(0, 1e-3, (70000, 3))).astype(np.float32)
    out = run(ctx, big, fixed, None, None, mode, LIMIT)
    assert same_outputs(out, run(ctx, big, fixed, None, None, mode, LIMIT))
    fitness, rmse, sums, info, idx, d2 = out
    kidx, kd2 = ctx.knn_search(big, fixed, 1, mode, LIMIT)
    assert np.array_equal(idx, kidx[:, 0]) and np.array_equal(bits(d2), bits(kd2[:, 0])) and sums[29] == 70000
    want, mags = E.sums_of_pairs(P.move_f32(np.eye(3), np.zeros(3), big), fixed, idx, kd2[:, 0])
    check_sums(sums, want, mags, 70000, "70000 points mode %d" % mode)
    check_derived(out, 70000, "70000 points mode %d" % mode)


# ---- 3. the pairs given
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("which", POSES)
def test_given_its_own_answer_search_mode_repeats_itself(ctx, which, mode):
    moving, fixed = scene("origin")[:2]
    for n in (65, 3000):
        searched = run(ctx, moving[:n], fixed, pose("origin", which), None, mode, POSE_LIMIT[which])
        given = run(ctx, moving[:n], fixed, pose("origin", which), searched[4], mode, POSE_LIMIT[which])
        assert same_outputs(searched, given), (which, mode, n)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", SCENES)
def test_given_pairs_against_the_restatement(ctx, name, mode):
    moving, fixed = scene(name)[:2]
    # the matches of the unregistered clouds, every seventh one withdrawn, under the true pose
    pairs = ctx.knn_search(moving, fixed, 1, mode)[0][:, 0].copy()
    pairs[::7] = -1
    ctx.profile_enable(True)
    try:
        out, ref = check(ctx, moving, fixed, pose(name, "truth"), mode, LIMIT, "%s given mode %d" % (name, mode), pairs=pairs)
        times = ctx.evaluate_registration_times()
    finally:
        ctx.profile_enable(False)
    assert times["grid"] == 0 and times["total"] > 0 and times["step"] > 0, times
    assert (out[4][::7] == -1).all() and np.isposinf(out[5][::7]).all() and 0 < out[0] <= 6 / 7 + 1e-3
    # a limit between the pairs' distances: those beyond it are dropped and show -1 / +inf
    cut = float(np.median(ref["d2"][np.isfinite(ref["d2"])]))
    out, ref = check(ctx, moving, fixed, pose(name, "truth"), mode, cut, "%s given, limited mode %d" % (name, mode), pairs=pairs)
    dropped = (pairs >= 0) & (out[4] == -1)
    assert 1000 < dropped.sum() < 1600 and np.isposinf(out[5][dropped]).all() and (out[5][out[4] >= 0] <= np.float32(cut)).all()
    # one pair alone, far beyond the limit; and n = 1 with no pair at all
    far = np.full(len(moving), -1, np.int32)
    far[17] = int(np.argmax(((fixed - moving[17]) ** 2).sum(axis=1)))
    out, _ = check(ctx, moving, fixed, None, mode, LIMIT, "%s one far pair mode %d" % (name, mode), pairs=far)
    assert out[0] == 0 and (out[4] == -1).all()
    check(ctx, moving[:1], fixed, None, mode, np.inf, "%s n = 1 withdrawn mode %d" % (name, mode), pairs=np.array([-1], np.int32))
    check(ctx, moving[:1], fixed[:1], None, mode, np.inf, "%s n = m = 1 mode %d" % (name, mode), pairs=np.array([0], np.int32))


# ---- 4. no pair at all is an answer
@pytest.mark.parametrize("mode", MODES)
def test_an_empty_answer(ctx, mode):
    moving, fixed = scene("origin")[:2]
    for pairs in (None, np.zeros(3000, np.int32)):
        fitness, rmse, sums, info, idx, d2 = run(ctx, moving + np.float32(10), fixed, None, pairs, mode, 0.0)
        assert fitness == 0.0 and rmse == 0.0 and (bits(sums) == 0).all() and (bits(info) == 0).all()
        assert (idx == -1).all() and np.isposinf(d2).all()
    # limit 0 keeps a pair at distance 0: a cloud against itself
    fitness, rmse = ctx.evaluate_registration(fixed, fixed, max_d2=0.0, dist_mode=mode, want_information=False)
    assert fitness == 1.0 and rmse == 0.0


# ---- 5. refusals on a live context
def test_invalid_arguments_are_refused_with_the_outputs_untouched(ctx, capi):
    """(MI_ERR_STATE on a distributed context: the suite has no fixture for one in this process; the refusal stands in eval_api.hip in front
    of MI_ENTER, the line every single-GPU entry point has.)"""
    moving, fixed = scene("origin")[:2]
    moving, fixed = moving[:200].copy(), fixed[:300].copy()
    n, m = len(moving), len(fixed)
    nan, inf = float("nan"), float("inf")
    good = np.arange(n, dtype=np.int32)

    def spoiled(a, row, value):
        a = a.copy()
        a[row, 1] = value
        return a

    def refused(what, before=moving, after=fixed, n=n, m=m, T=None, pairs=None, mode=0, max_d2=inf, null=()):
        fitness, rmse = C.c_double(-7.5), C.c_double(-7.5)
        sums, info, idx, d2 = np.full(32, -7.5), np.full(36, -7.5), np.full(len(before), -7, np.int32), np.full(len(before), -7.5, np.float32)
        ptr = {"before": before.ctypes.data, "after": after.ctypes.data, "fitness": C.addressof(fitness), "rmse": C.addressof(rmse)}
        for k in null:
            ptr[k] = None
        rc = capi.evaluate_registration_raw(ctx._h, ptr["before"], n, ptr["after"], m, None if T is None else T.ctypes.data,
                                            None if pairs is None else pairs.ctypes.data, mode, max_d2, ptr["fitness"], ptr["rmse"], sums.ctypes.data,
                                            info.ctypes.data, idx.ctypes.data, d2.ctypes.data)
        msg = capi.lib().mi_last_error().decode()
        assert rc == capi.MI_ERR_INVALID_ARG and msg.startswith("mi_evaluate_registration:"), (what, rc, msg)
        assert fitness.value == -7.5 and rmse.value == -7.5, what
        assert (sums == -7.5).all() and (info == -7.5).all() and (idx == -7).all() and (d2 == -7.5).all(), what
        return msg

    for k in ("before", "after", "fitness", "rmse"):
        refused("null " + k, null=(k,))
    refused("n = 0", n=0)
    refused("m = 0", m=0)
    refused("n negative", n=-3)
    refused("dist_mode", mode=2)
    refused("limit nan", max_d2=nan)
    refused("limit negative", max_d2=-1.0)
    bad = np.eye(4, dtype=np.float32).reshape(16)
    bad[13] = inf
    assert "entry 13" in refused("transform", T=bad)
    assert "before_xyz point 17" in refused("before nan", before=spoiled(moving, 17, nan))
    assert "after_xyz point 5" in refused("after inf", after=spoiled(fixed, 5, inf))
    assert "after_xyz point 6" in refused("after large", after=spoiled(fixed, 6, 2e18), pairs=good)
    for value in (m, -2, 2 ** 31 - 1, -2 ** 31):
        pairs = good.copy()
        pairs[[150, 31, 90]] = value
        assert "pair_idx entry 31 " in refused("pair %d" % value, pairs=pairs), value
    pairs = good.copy()
    pairs[n - 1] = m
    assert "pair_idx entry %d " % (n - 1) in refused("last pair", pairs=pairs)
    # the bottom row of a transform is never read; m - 1 and -1 are good pairs; and the context still works
    loose = np.eye(4, dtype=np.float32)
    loose[3] = nan
    assert same_outputs(run(ctx, moving, fixed, loose), run(ctx, moving, fixed))
    pairs = good.copy()
    pairs[0], pairs[1] = m - 1, -1
    assert run(ctx, moving, fixed, None, pairs)[4].tolist() == pairs.tolist()


# ---- 6. history
def test_a_loaded_icp_problem_survives(ctx, capi, bunny):
    before, after = bunny
    moving, fixed = scene("origin")[:2]
    params = capi.icp_params(eps=1e-9, max_iterations=12)

    def icp(between):
        ctx.icp_load(before, after, params)
        ctx.icp_run(5)
        if between:
            found = run(ctx, moving, fixed, None, None, K.DIST_CPU_ROUNDING, LIMIT)
            run(ctx, moving, fixed, None, found[4], K.DIST_CPU_ROUNDING, LIMIT)
        ctx.icp_run(7)
        R, t, it, err, why = ctx.icp_result()
        return bits(R).tolist(), bits(t).tolist(), it, bits(np.float32(err)).tolist(), why

    assert icp(True) == icp(False)


def test_same_bits_whatever_ran_before(ctx, capi):
    moving, fixed, normals, G = scene("origin")
    T = pose("origin", "off")
    first = run(ctx, moving, fixed, T, None, K.DIST_CPU_ROUNDING, LIMIT * LIMIT)
    ctx.icp_plane_register(moving, fixed, normals, capi.plane_params(max_distance_squared=LIMIT))
    assert same_outputs(run(ctx, moving, fixed, T, None, K.DIST_CPU_ROUNDING, LIMIT * LIMIT), first)
    ctx.knn_search(None, fixed, 8)
    run(ctx, moving[:100], fixed[:50], None, np.zeros(100, np.int32))
    assert same_outputs(run(ctx, moving, fixed, T, None, K.DIST_CPU_ROUNDING, LIMIT * LIMIT), first)


def test_no_buffer_outlives_its_context(capi, ctx):
    """(the session's context keeps its own buffers: the count goes back to where it was, 0 of this context's left)"""
    moving, fixed = scene("origin")[:2]
    start = capi.selftest_live_buffers()
    with capi.Context(0) as own:
        own.profile_enable(True)
        found = run(own, moving, fixed, None, None, K.DIST_CPU_ROUNDING, LIMIT)
        run(own, moving, fixed, None, found[4], K.DIST_CPU_ROUNDING, LIMIT)
        assert capi.selftest_live_buffers() > start
    assert capi.selftest_live_buffers() - start == 0


# ---- 7. consistency with what exists
@pytest.mark.parametrize("mode", MODES)
def test_the_pairs_are_the_plane_systems(ctx, mode):
    """Every normal of the scene is non-zero, so mi_plane_system takes the same pairs in the same order: its count and its sum of d2 are
    this call's, bit for bit."""
    moving, fixed, normals, _ = scene("origin")
    for which in POSES:
        T = pose("origin", which)
        plane = ctx.plane_system(moving, fixed, normals, T, mode, POSE_LIMIT[which])
        out = run(ctx, moving, fixed, T, None, mode, POSE_LIMIT[which])
        assert out[2][29] == plane[0][29] and bits(out[2][28:29]) == bits(plane[0][28:29]), which
        assert np.array_equal(out[4], plane[2]), which


def test_the_system_is_a_gauss_newton_step(ctx):
    """Lambda x = -g of the device's sums at the pose 0.3 off, applied about the origin, brings the restatement's sum |d|^2 over the same
    pairs down."""
    moving, fixed = scene("origin")[:2]
    T = pose("origin", "off")
    fitness, rmse, sums, info, idx, d2 = run(ctx, moving, fixed, T, None, K.DIST_CPU_ROUNDING, LIMIT * LIMIT)
    x = np.linalg.solve(info, -sums[21:27])
    R, t = pose_of(T)
    dR = P.rodrigues(x[:3])
    before = E.evaluate(moving, fixed, R, t, pairs=idx)
    after = E.evaluate(moving, fixed, dR @ R, dR @ t + x[3:], pairs=idx)
    print("sum |d|^2 over %d pairs: %.6f -> %.6f" % (int(sums[29]), before["sums"][27], after["sums"][27]))
    assert before["sums"][29] == after["sums"][29] == sums[29] and after["sums"][27] < before["sums"][27]
