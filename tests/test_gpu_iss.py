"""GPU suite of mi_iss_keypoints against the float64 restatement of tests/iss_reference.py, stage by stage.  The restatement of a main
cloud is built once per cloud and arithmetic (lru_cache) and shared, unchanged, by every test that needs it.

The bounds (none of them taken from what the device gives):
  neighbours    equal to the restatement's
  eigenvalues   |got - lambda_ref| <= 6e-8 |lambda_ref| + 8 (count + 8) 2^-53 r_s^2: one fp32 rounding (2^-24 = 5.96e-8), and the linear
                worst case of `count` fp64 additions of terms bounded by r_s^2, plus the Jacobi's backward error
  gate          read as saliency > 0: equal on every point that is below min_neighbours on both sides (the counts are equal) or whose
                two ratio tests are clear of their gamma by more than 1e-9, relative to the larger eigenvalue of the test -- and, where
                the gate holds, whose lambda0 is further from 0 than its own bound above (gate_decided: a scatter of rank < 3 has a
                lambda0 of either sign).  On the three main clouds the restatement alone shows that this leaves no point out: the
                smallest margin is 9.8e-5
  saliency      where both sides pass the gate, within the same bound as lambda0
  suppression   is_keypoint == iss_reference.nms(the device's OWN saliency), exactly
  consistency   out_index = flatnonzero(is_keypoint), out_xyz = the bits of cloud[out_index], out_n = is_keypoint.sum(); asking for fewer
                optional outputs gives the same bits in the rest; two calls give the same bits whatever ran in between"""
import ctypes as C
import functools

import numpy as np
import pytest

import iss_reference as I
import knn_reference as K

pytestmark = pytest.mark.gpu

MODES = (K.DIST_CPU_ROUNDING, K.DIST_FMA)
MAIN = {"surface": (0.9, 0.6), "volume": (1.6, 1.1), "offset": (0.9, 0.6)}     # salient and non-max radius
KEYPOINTS = {"surface": 40, "volume": 134, "offset": 40}                       # what the restatement alone gives
OUTPUTS = ("is_keypoint", "saliency", "eigenvalues", "neighbours")


def frozen(a):
    a.setflags(write=False)
    return a


def surface_recipe(rng, n_surface, n_stray, half):
    xy = rng.uniform(-half, half, (n_surface, 2))
    z = 0.6 * np.sin(1.3 * xy[:, 0]) * np.cos(1.1 * xy[:, 1]) + 0.01 * rng.normal(size=n_surface)
    return np.concatenate([np.concatenate([xy, z[:, None]], axis=1), rng.uniform(-half, half, (n_stray, 3))]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def clouds():
    rng = np.random.default_rng(97)
    surface = surface_recipe(rng, 2400, 100, 5)
    volume = rng.uniform(-5, 5, (2500, 3)).astype(np.float32)
    offset = (surface + np.array([100.0, -50.0, 25.0], np.float32)).astype(np.float32)
    return {"surface": frozen(surface), "volume": frozen(volume), "offset": frozen(offset)}


@functools.lru_cache(maxsize=None)
def reference(name, mode):
    ref, key = I.keypoints(clouds()[name], MAIN[name][0], MAIN[name][1], mode)
    return {k: frozen(v) for k, v in ref.items()}, frozen(key)


def lattice(side):
    g = np.arange(side, dtype=np.float32)
    z, y, x = np.meshgrid(g, g, g, indexing="ij")
    return np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1)       # index = x + side y + side^2 z


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype.itemsize == 4 else a


def run(ctx, capi, cloud, want=OUTPUTS, **fields):
    """One call -> dict of everything that was asked for."""
    res = list(ctx.iss_keypoints(cloud, capi.iss_params(**fields), **{"want_" + name: name in want for name in OUTPUTS}))
    out = {"xyz": res.pop(0), "index": res.pop(0)}
    for name in OUTPUTS:
        if name in want:
            out[name] = res.pop(0)
    return out


def same_bits(a, b):
    """every output the two answers share, bit for bit"""
    return all(np.array_equal(bits(a[name]), bits(b[name])) for name in set(a) & set(b))


def check_consistency(cloud, got, what):
    flag = got["is_keypoint"]
    assert set(np.unique(flag).tolist()) <= {0, 1}, what
    assert np.array_equal(got["index"], np.flatnonzero(flag).astype(np.int32)), what
    assert got["xyz"].shape == (len(got["index"]), 3) and np.array_equal(bits(got["xyz"]), bits(cloud[got["index"]])), what
    assert len(got["index"]) == int(flag.sum()), what


def gate_decided(ref, min_neighbours, lambda0_bound):
    """The points on which "saliency > 0" is decided by the restatement alone: below min_neighbours (the counts are equal); or both ratio
    tests clear of their gamma by more than 1e-9 and then either the gate fails (+0 on both sides) or lambda0 is further from 0 than its
    own error bound -- a scatter of rank < 3 (two neighbours, an exact plane) has lambda0 = 0 to rounding, of either sign."""
    clear = ref["margin"] > 1e-9
    return (ref["count"] < min_neighbours) | (clear & (~ref["gate"] | (np.abs(ref["lam"][:, 0]) > lambda0_bound)))


def check_stage_1(got, ref, salient_radius, min_neighbours, what, only=None, cap=False):
    """K32's outputs against the restatement's (of the rows `only` alone where given); returns the points left out of the gate check."""
    pick = (lambda a: a) if only is None else (lambda a: a[only])
    count, lam = ref["count"], ref["lam"]
    assert np.array_equal(pick(got["neighbours"]), count), what
    slack = 8.0 * (count + 8) * 2.0 ** -53 * float(np.float32(salient_radius)) ** 2
    err = np.abs(pick(got["eigenvalues"]).astype(np.float64) - lam)
    bound = 6e-8 * np.abs(lam) + slack[:, None]
    decided = gate_decided(ref, min_neighbours, bound[:, 0])
    gate = pick(got["saliency"]) > 0
    both = gate & ref["gate"] & (ref["saliency"] > 0)
    serr = np.abs(pick(got["saliency"]).astype(np.float64) - lam[:, 0])
    print("%s: eigenvalues worst error / bound %.3f; %d candidates (restatement %d); left out of the gate check %d; saliency worst error / bound %.3f" % (
        what, (err / np.maximum(bound, 1e-300)).max(initial=0.0), gate.sum(), (ref["saliency"] > 0).sum(), (~decided).sum(),
        (serr[both] / bound[both, 0]).max(initial=0.0)))
    assert (err <= bound).all(), what
    assert (pick(got["eigenvalues"])[count == 0] == 0).all(), what
    if cap:
        assert decided.all(), what                                    # (the restatement alone)
    assert np.array_equal(gate[decided], (ref["saliency"] > 0)[decided]), what
    assert (pick(got["saliency"]) >= 0).all() and not np.signbit(pick(got["saliency"])).any(), what
    assert (serr[both] <= bound[both, 0]).all(), what
    return int((~decided).sum())


def check_stage_2(cloud, got, non_max_radius, min_neighbours, mode, what, only=None):
    """K33 exactly: the flags are the restatement's suppression of the DEVICE's saliency."""
    want = I.nms(got["saliency"], cloud, non_max_radius, min_neighbours, mode, only=only)
    flag = got["is_keypoint"].astype(bool)
    assert np.array_equal(flag if only is None else flag[only], want), what


def fewer_outputs_agree(ctx, capi, cloud, full, **fields):
    assert same_bits(run(ctx, capi, cloud, want=(), **fields), full), fields
    assert same_bits(run(ctx, capi, cloud, want=("is_keypoint",), **fields), full), fields
    assert same_bits(run(ctx, capi, cloud, want=("saliency", "neighbours"), **fields), full), fields
    assert same_bits(run(ctx, capi, cloud, want=("eigenvalues",), **fields), full), fields


# ---- 1. the three main clouds, both arithmetics: stage 1, stage 2, consistency, determinism
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(MAIN))
def test_main_clouds_stage_by_stage(ctx, capi, name, mode):
    cloud, (rs, rn) = clouds()[name], MAIN[name]
    ref, ref_key = reference(name, mode)
    # the restatement alone, before looking at the device
    assert int(ref_key.sum()) == KEYPOINTS[name]
    assert ((ref["count"] < 5) | (ref["margin"] > 1e-9)).all() and ref["margin"][ref["count"] >= 5].min() > 9.7e-5
    assert gate_decided(ref, 5, 6e-8 * np.abs(ref["lam"][:, 0]) + 8.0 * (ref["count"] + 8) * 2.0 ** -53 * float(np.float32(rs)) ** 2).all()
    cand = ref["saliency"][ref["saliency"] > 0]
    if name == "surface":
        assert round(float(ref["count"].mean())) == 50 and int((ref["count"] < 5).sum()) == 81
        assert (len(cand), len(cand) - len(np.unique(cand))) == (2405, 47)          # the tie rule is exercised
    if name == "volume":
        assert round(float(ref["count"].mean())) == 35
    fields = dict(salient_radius=rs, non_max_radius=rn, dist_mode=mode)
    what = "%s mode %d" % (name, mode)
    got = run(ctx, capi, cloud, **fields)
    assert check_stage_1(got, ref, rs, 5, what, cap=True) == 0
    dev = got["saliency"][got["saliency"] > 0]
    print("%s: the device's saliency repeats %d values among %d candidates" % (what, len(dev) - len(np.unique(dev)), len(dev)))
    check_stage_2(cloud, got, rn, 5, mode, what)
    check_consistency(cloud, got, what)
    diff = np.flatnonzero(got["is_keypoint"].astype(bool) != ref_key)
    print("%s: %d keypoints (restatement %d), symmetric difference %s" % (what, len(got["index"]), ref_key.sum(), diff.tolist()))
    assert 0 < len(got["index"]) < len(cloud) // 10
    fewer_outputs_agree(ctx, capi, cloud, got, **fields)
    ctx.knn_search(None, clouds()["volume"][:777], 8, K.DIST_FMA)
    assert same_bits(run(ctx, capi, cloud, **fields), got), what


# ---- 2. the smallest shapes and the ends of a wave
@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 129])
def test_smallest_shapes(ctx, capi, n):
    rng = np.random.default_rng(2000 + n)
    half = 0.4 if n <= 3 else 1.0                                       # (two or three points: close enough to be each other's neighbours)
    cloud = rng.uniform(-half, half, (n, 3)).astype(np.float32)
    left_out = 0
    for mode in MODES:
        for rs, rn, min_nb in ((0.9, 0.6, 3), (0.6, 0.9, 1)):
            fields = dict(salient_radius=rs, non_max_radius=rn, min_neighbours=min_nb, dist_mode=mode)
            what = "n %d radii %g %g mode %d" % (n, rs, rn, mode)
            got = run(ctx, capi, cloud, **fields)
            left_out += check_stage_1(got, I.saliency(cloud, rs, mode, min_neighbours=min_nb), rs, min_nb, what)
            check_stage_2(cloud, got, rn, min_nb, mode, what)
            check_consistency(cloud, got, what)
            fewer_outputs_agree(ctx, capi, cloud, got, **fields)
            if n == 1:
                assert got["neighbours"].tolist() == [0] and got["eigenvalues"].tolist() == [[0.0, 0.0, 0.0]] and got["saliency"].tolist() == [0.0]
    print("n %d: %d points left out of the gate checks" % (n, left_out))


# ---- 3. clouds without a candidate
@pytest.mark.parametrize("mode", MODES)
def test_identical_points_and_an_exact_plane_have_no_keypoint(ctx, capi, mode):
    same = np.tile(np.array([[1.5, -2.25, 3.0]], np.float32), (200, 1))
    got = run(ctx, capi, same, salient_radius=1.0, non_max_radius=1.0, dist_mode=mode)
    assert (got["neighbours"] == 199).all() and (got["eigenvalues"] == 0).all() and (bits(got["saliency"]) == 0).all()
    assert len(got["index"]) == 0 and not got["is_keypoint"].any()
    check_consistency(same, got, "identical")
    rng = np.random.default_rng(5)
    plane = rng.uniform(-5, 5, (400, 3)).astype(np.float32)
    plane[:, 2] = 0.75
    got = run(ctx, capi, plane, salient_radius=1.5, non_max_radius=1.0, dist_mode=mode)
    ref = I.saliency(plane, 1.5, mode)
    check_stage_1(got, ref, 1.5, 5, "plane mode %d" % mode)
    assert (got["eigenvalues"][:, 0] == 0).all() and (got["eigenvalues"][:, 2] > 0).all()      # lambda0 = 0 exactly
    assert (bits(got["saliency"]) == 0).all() and len(got["index"]) == 0 and not got["is_keypoint"].any()
    check_consistency(plane, got, "plane")


# ---- 4. exact ties everywhere: the 5 x 5 x 5 lattice
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("radius", [1.0, float(np.nextafter(np.sqrt(np.float32(2)), np.float32(2)))])
def test_lattice_with_exact_ties(ctx, capi, radius, mode):
    L = lattice(5)
    # (sqrt 2: the fp32 root's square rounds to the float below 2, so the radius is the next float up, whose square is the float above 2:
    # the points at d2 = 2 belong)
    assert np.sqrt(np.float32(2)) * np.sqrt(np.float32(2)) < 2 <= np.float32(radius) * np.float32(radius) < 2.000001 or radius == 1.0
    for min_nb in (1, 4):
        fields = dict(salient_radius=radius, non_max_radius=radius, min_neighbours=min_nb, dist_mode=mode)
        what = "lattice 5 radius %g min %d mode %d" % (radius, min_nb, mode)
        got = run(ctx, capi, L, **fields)
        ref = I.saliency(L, radius, mode, min_neighbours=min_nb)
        left_out = check_stage_1(got, ref, radius, min_nb, what)
        dev = got["saliency"][got["saliency"] > 0]
        print("%s: %d left out, the device's saliency repeats %d values among %d candidates, %d keypoints" % (
            what, left_out, len(dev) - len(np.unique(dev)), len(dev), len(got["index"])))
        check_stage_2(L, got, radius, min_nb, mode, what)
        check_consistency(L, got, what)
        fewer_outputs_agree(ctx, capi, L, got, **fields)
    on_boundary = ((L == 0) | (L == 4)).sum(axis=1)
    if radius == 1.0:
        assert np.array_equal(run(ctx, capi, L, salient_radius=1.0, non_max_radius=1.0, dist_mode=mode)["neighbours"], 6 - on_boundary)


# ---- 5. the radii the other way round, a ball that holds the whole cloud, a threshold nobody reaches
@pytest.mark.parametrize("mode", MODES)
def test_radii_and_thresholds_at_their_ends(ctx, capi, mode):
    cloud = clouds()["surface"][::5]                                    # 500 points
    n = len(cloud)
    for rs, rn, min_nb in ((0.9, 2.5, 5), (40.0, 1.5, 5), (1.5, 40.0, 5), (1.5, 1.0, n), (40.0, 40.0, n - 1)):
        fields = dict(salient_radius=rs, non_max_radius=rn, min_neighbours=min_nb, dist_mode=mode)
        what = "radii %g %g min %d mode %d" % (rs, rn, min_nb, mode)
        got = run(ctx, capi, cloud, **fields)
        check_stage_1(got, I.saliency(cloud, rs, mode, min_neighbours=min_nb), rs, min_nb, what)
        check_stage_2(cloud, got, rn, min_nb, mode, what)
        check_consistency(cloud, got, what)
        if rs == 40.0:
            assert (got["neighbours"] == n - 1).all(), what             # every point's ball is the whole cloud
        if rn == 40.0 and min_nb == 5:
            assert len(got["index"]) == 1, what                         # one maximum of the whole cloud (the lowest index of a tie)
        if min_nb == n:
            assert len(got["index"]) == 0 and not got["is_keypoint"].any() and (bits(got["saliency"]) == 0).all(), what    # above n - 1: MI_OK, nothing


# ---- 6. beyond one grid layer per axis
@functools.lru_cache(maxsize=None)
def wide_surface():
    cloud = frozen(surface_recipe(np.random.default_rng(97), 19200, 800, 15))
    sample = frozen(np.sort(np.random.default_rng(98).permutation(len(cloud))[:256]))
    return cloud, sample


@pytest.mark.parametrize("mode", MODES)
def test_a_surface_of_20000_points_on_sampled_rows(ctx, capi, mode):
    cloud, sample = wide_surface()
    fields = dict(salient_radius=0.9, non_max_radius=0.6, dist_mode=mode)
    got = run(ctx, capi, cloud, **fields)
    ref = I.saliency(cloud, 0.9, mode, only=sample)
    assert ref["count"].mean() > 30
    what = "wide surface mode %d" % mode
    check_stage_1(got, ref, 0.9, 5, what, only=sample)
    # (a sampled row of the distance matrix covers its point's whole non-max ball, and the device's saliency is known for every point)
    check_stage_2(cloud, got, 0.6, 5, mode, what, only=sample)
    check_consistency(cloud, got, what)
    assert 0 < len(got["index"]) < len(cloud) // 10


# ---- 7. context hygiene
def test_a_loaded_icp_problem_survives(ctx, capi, golden):
    z = golden.npz("synth2k_clouds.npz")
    params = capi.icp_params(max_iterations=8)
    ctx.icp_load(z["before"], z["after"], params)
    ctx.icp_run(8)
    R0, t0, it0, err0, why0 = ctx.icp_result()
    ctx.icp_load(z["before"], z["after"], params)
    got = run(ctx, capi, clouds()["offset"], salient_radius=0.9, non_max_radius=0.6, dist_mode=K.DIST_FMA)
    assert len(got["index"]) > 0
    ctx.icp_run(8)
    R1, t1, it1, err1, why1 = ctx.icp_result()
    assert it0 > 0 and (it1, why1) == (it0, why0)
    assert np.array_equal(bits(R1), bits(R0)) and np.array_equal(bits(t1), bits(t0))
    assert np.float32(err1).tobytes() == np.float32(err0).tobytes()


# ---- 8. refusals: nothing is written
def raw_call(ctx, capi, cloud, n, null_params=False, null_out_n=False, **fields):
    """mi_iss_keypoints with every output prefilled with a sentinel -> (error code, message, outputs untouched?)"""
    rows = max(n, 1)
    xyz, index, flag = np.full(3 * rows, -7.5, np.float32), np.full(rows, -7, np.int32), np.full(rows, 7, np.uint8)
    saliency, eigenvalues, neighbours = np.full(rows, -7.5, np.float32), np.full(3 * rows, -7.5, np.float32), np.full(rows, -7, np.int32)
    out_n = C.c_int(-7)
    p = capi.iss_params(**dict(dict(salient_radius=0.9, non_max_radius=0.6), **fields))
    rc = capi.iss_keypoints_raw(ctx._h, None if cloud is None else cloud.ctypes.data, n, None if null_params else C.addressof(p), xyz.ctypes.data,
                                index.ctypes.data, None if null_out_n else C.addressof(out_n), flag.ctypes.data, saliency.ctypes.data,
                                eigenvalues.ctypes.data, neighbours.ctypes.data)
    untouched = bool((xyz == -7.5).all() and (index == -7).all() and (flag == 7).all() and (saliency == -7.5).all() and (eigenvalues == -7.5).all()
                     and (neighbours == -7).all() and out_n.value == -7)
    return rc, capi.lib().mi_last_error().decode(), untouched


def test_refusals_leave_the_outputs_untouched(ctx, capi):
    c = np.array(clouds()["surface"][:1000])
    nan, inf = float("nan"), float("inf")
    bad_args = [dict(cloud=None, n=1000), dict(cloud=c, n=1000, null_params=True), dict(cloud=c, n=1000, null_out_n=True),
                dict(cloud=c, n=0), dict(cloud=c, n=-1), dict(cloud=c, n=1000, dist_mode=2), dict(cloud=c, n=1000, dist_mode=-1),
                dict(cloud=c, n=1000, min_neighbours=0), dict(cloud=c, n=1000, min_neighbours=-3)]
    for field in ("salient_radius", "non_max_radius"):
        bad_args += [dict(cloud=c, n=1000, **{field: v}) for v in (nan, inf, 0.0, -1.0, 1e20)]      # (1e20: the square is not finite)
    for field in ("gamma_21", "gamma_32"):
        bad_args += [dict(cloud=c, n=1000, **{field: v}) for v in (nan, inf, 0.0, -0.5)]
    for kw in bad_args:
        rc, msg, untouched = raw_call(ctx, capi, **kw)
        assert rc == capi.MI_ERR_INVALID_ARG and untouched and msg.startswith("mi_iss_keypoints"), (kw, msg)
        named = [k for k in kw if k not in ("cloud", "n", "null_params", "null_out_n")]
        assert all(k in msg for k in named), (kw, msg)                  # the cause: the field's name
    # a bad point: its index -- the LOWEST one
    for value in (np.nan, np.inf, -np.inf, 1.5e18, -1.5e18):
        bc = c.copy()
        bc[917, 2] = value
        bc[333, 0] = value
        rc, msg, untouched = raw_call(ctx, capi, bc, 1000)
        assert rc == capi.MI_ERR_INVALID_ARG and untouched and msg.startswith("mi_iss_keypoints") and "cloud_xyz point 333 " in msg, (value, msg)
    with pytest.raises(capi.MiSlamError) as e:
        bc = c.copy()
        bc[5, 0] = np.nan
        ctx.iss_keypoints(bc, capi.iss_params(salient_radius=0.9, non_max_radius=0.6))
    assert "cloud_xyz point 5 " in str(e.value)
    # and the context still works
    ref, _ = reference("surface", K.DIST_CPU_ROUNDING)
    got = run(ctx, capi, clouds()["surface"], salient_radius=0.9, non_max_radius=0.6)
    check_stage_1(got, ref, 0.9, 5, "after the refusals", cap=True)
    check_stage_2(clouds()["surface"], got, 0.6, 5, K.DIST_CPU_ROUNDING, "after the refusals")
