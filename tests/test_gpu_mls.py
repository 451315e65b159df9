"""GPU suite of mi_mls_smooth against the float64 restatement of tests/mls_reference.py.  The restatement of a main case is built once
(tests/mls_cases.py, lru_cache) and shared, unchanged, by every test that needs it.

The bounds (none of them taken from what the device gives):
  neighbours    equal to the restatement's
  status        equal on every query the restatement decides: its own scaled smallest pivot is not within a factor 10 of the pivot floor
                1e-10 (c = 6 is not treated apart).  On the main clouds the restatement alone shows that every query is decided
                (tests/test_mls_bound.py)
  curvature     tests/test_gpu_iss.py's eigenvalue bound, on the eigenvalue the curvature stands for: | curvature x trace_ref - max(lambda0_ref, 0) |
                <= 6e-8 lambda0_ref + 8 (c + 8) 2^-53 r^2 -- one fp32 rounding and the linear worst case of c fp64 additions of terms bounded by
                r^2, plus the Jacobi's backward error
  out_xyz,      per coordinate half an fp32 ulp of the reference value plus K (c + 8) 2^-53 radius / conditioning, the normal up to its
  out_normals   sign; conditioning (mls_reference.conditioning): the restatement's scaled smallest pivot where the quadratic answered, the
                eigenvalue gap (lambda1 - lambda0) / radius^2 where the plane did (order 1, fewer than six points: the plane's normal is
                held by that gap alone).  K = 5.7: four times the worst spread of the restatement between ascending and descending
                summation over the main cases, measured 1.41 (tests/test_mls_bound.py).  Queries conditioned below 1e-6 are left out; on
                the main clouds none is (at most 1 % may be)
  untouched     out_xyz is the query's input bits, the normal (0, 0, 0), the curvature 0
  consistency   asking for fewer optional outputs gives the same bits in the rest; two calls give the same bits whatever ran in between"""
import ctypes as C
import functools

import numpy as np
import pytest

import knn_reference as K
import mls_cases as S
import mls_reference as M
import search_scale_cases as scale
from test_gpu_iss import bits, clouds, frozen, same_bits, wide_surface

pytestmark = pytest.mark.gpu

MODES = (K.DIST_CPU_ROUNDING, K.DIST_FMA)
OUTPUTS = ("normals", "curvature", "neighbours", "status")
U = 2.0 ** -53


def run(ctx, capi, cloud, queries=None, want=OUTPUTS, **fields):
    """One call -> dict of everything that was asked for."""
    res = ctx.mls_smooth(cloud, capi.mls_params(**fields), queries=queries, **{"want_" + name: name in want for name in OUTPUTS})
    res = list(res) if isinstance(res, tuple) else [res]
    out = {"xyz": res.pop(0)}
    for name in OUTPUTS:
        if name in want:
            out[name] = res.pop(0)
    return out


def half_ulp32(x):
    x = np.abs(np.asarray(x, np.float64)).astype(np.float32)
    return 0.5 * (np.nextafter(x, np.float32(np.inf)).astype(np.float64) - x.astype(np.float64))


def check(got, ref, queries, radius, what, only=None):
    """Every output against the restatement's (of the rows `only` alone where given); returns the queries left out of the coordinate check."""
    pick = (lambda a: a) if only is None else (lambda a: a[only])
    q = np.ascontiguousarray(queries, np.float32) if only is None else np.ascontiguousarray(queries, np.float32)[only]
    count, status = ref["neighbours"], ref["status"]
    assert np.array_equal(pick(got["neighbours"]), count), what
    decided = ~((ref["pivot"] > M.PIVOT_MIN / 10) & (ref["pivot"] < M.PIVOT_MIN * 10))
    assert np.array_equal(pick(got["status"])[decided], status[decided]), what
    assert set(np.unique(got["status"]).tolist()) <= {0, 1, 2}, what
    same = pick(got["status"]) == status
    untouched = status == M.UNTOUCHED
    assert np.array_equal(bits(pick(got["xyz"])[untouched]), bits(q[untouched])), what
    assert (bits(pick(got["normals"])[untouched]) == 0).all() and (bits(pick(got["curvature"])[untouched]) == 0).all(), what
    r = float(np.float32(radius))
    # the curvature, as the eigenvalue it stands for
    trace = ref["lam"].sum(axis=1)
    lam0 = np.maximum(ref["lam"][:, 0], 0.0)
    cerr = np.abs(pick(got["curvature"]).astype(np.float64) * trace - np.where(untouched, 0.0, lam0))
    cbound = 6e-8 * lam0 + 8.0 * (count + 8) * U * r * r
    assert (cerr <= cbound).all(), (what, (cerr / cbound).max())
    assert (pick(got["curvature"]) >= 0).all() and (pick(got["curvature"]) <= np.float32(1.0 / 3.0) * np.float32(1 + 1e-6)).all(), what
    # the coordinates
    rows = S.checked(ref, radius) & same
    unit = M.error_unit(ref, radius)
    xerr = np.abs(pick(got["xyz"]).astype(np.float64) - ref["xyz64"])
    xbound = half_ulp32(ref["xyz64"]) + (S.K_BOUND * unit)[:, None]
    sign = np.where((pick(got["normals"]).astype(np.float64) * ref["normals64"]).sum(axis=1) >= 0, 1.0, -1.0)[:, None]
    nerr = np.abs(pick(got["normals"]).astype(np.float64) - sign * ref["normals64"])
    nbound = half_ulp32(ref["normals64"]) + (S.K_BOUND * unit)[:, None]
    left_out = int(((status != M.UNTOUCHED) & ~rows).sum())
    print("%s: status counts %s (restatement %s), undecided %d, left out of the coordinate check %d; worst error / bound: curvature %.3f, xyz %.3f, normals %.3f; "
          "worst error in units of (c + 8) 2^-53 radius / conditioning beyond the fp32 half ulp: xyz %.3f, normals %.3f" % (
              what, np.bincount(pick(got["status"]), minlength=3).tolist(), np.bincount(status, minlength=3).tolist(), int((~decided).sum()), left_out,
              (cerr / cbound).max(initial=0.0), (xerr[rows] / xbound[rows]).max(initial=0.0), (nerr[rows] / nbound[rows]).max(initial=0.0),
              (np.maximum(xerr - half_ulp32(ref["xyz64"]), 0)[rows] / unit[rows][:, None]).max(initial=0.0),
              (np.maximum(nerr - half_ulp32(ref["normals64"]), 0)[rows] / unit[rows][:, None]).max(initial=0.0)))
    assert (xerr[rows] <= xbound[rows]).all(), what
    assert (nerr[rows] <= nbound[rows]).all(), what
    fitted = pick(got["status"]) != M.UNTOUCHED
    length = np.sqrt((pick(got["normals"]).astype(np.float64) ** 2).sum(axis=1))
    assert (np.abs(length[fitted] - 1) <= 2e-7).all() and np.isfinite(pick(got["xyz"])).all(), what
    return left_out


def fewer_outputs_agree(ctx, capi, cloud, queries, full, **fields):
    assert same_bits(run(ctx, capi, cloud, queries, want=(), **fields), full), fields
    assert same_bits(run(ctx, capi, cloud, queries, want=("status",), **fields), full), fields
    assert same_bits(run(ctx, capi, cloud, queries, want=("normals", "neighbours"), **fields), full), fields
    assert same_bits(run(ctx, capi, cloud, queries, want=("curvature",), **fields), full), fields


# ---- 1. the three main clouds, self mode and queries of their own, both arithmetics, both orders
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("separate", [False, True], ids=["self", "queries"])
@pytest.mark.parametrize("name", list(S.RADIUS))
def test_main_clouds(ctx, capi, name, separate, mode, order):
    cloud, radius = clouds()[name], S.RADIUS[name]
    queries = S.queries(name) if separate else None
    ref = S.reference(name, separate, mode, order)
    # the restatement alone, before looking at the device
    fitted = ref["status"] != M.UNTOUCHED
    assert (fitted & ~S.checked(ref, radius)).sum() <= S.LEFT_OUT_SHARE * len(fitted) and fitted.mean() > 0.9
    assert (ref["status"][fitted] == (M.QUADRATIC if order == 2 else M.PLANE)).mean() > 0.99
    fields = dict(radius=radius, dist_mode=mode, order=order)
    what = "%s %s mode %d order %d" % (name, "queries" if separate else "self", mode, order)
    got = run(ctx, capi, cloud, queries, **fields)
    check(got, ref, cloud if queries is None else queries, radius, what)
    if not separate:
        # the ball is mi_remove_outliers' radius count, plus the point itself
        nb = ctx.remove_outliers(cloud, capi.outlier_params(method=capi.OUTLIER_RADIUS, radius=radius, min_neighbours=1, dist_mode=mode), want_neighbours=True)[2]
        assert np.array_equal(got["neighbours"], nb + 1), what
    fewer_outputs_agree(ctx, capi, cloud, queries, got, **fields)
    ctx.knn_search(None, clouds()["volume"][:777], 8, K.DIST_FMA)
    assert same_bits(run(ctx, capi, cloud, queries, **fields), got), what


# ---- 2. the smallest shapes: the status boundaries at 3 and 6, the ends of a wave and of a block
@pytest.mark.parametrize("n", [1, 2, 3, 5, 6, 7, 63, 64, 65, 129])
def test_smallest_shapes(ctx, capi, n):
    rng = np.random.default_rng(3000 + n)
    cloud = np.concatenate([rng.uniform(-1, 1, (n, 2)), 0.05 * rng.normal(size=(n, 1))], axis=1).astype(np.float32)
    queries = (cloud[rng.integers(0, n, 40)] + rng.normal(scale=0.05, size=(40, 3))).astype(np.float32)
    left_out = 0
    for mode in MODES:
        for order in (1, 2):
            for q in (None, queries):
                fields = dict(radius=4.0, dist_mode=mode, order=order)                     # the ball holds the whole cloud
                what = "n %d mode %d order %d %s" % (n, mode, order, "self" if q is None else "queries")
                got = run(ctx, capi, cloud, q, **fields)
                ref = M.smooth(cloud, 4.0, mode, queries=q, order=order)
                assert (ref["neighbours"] == n).all(), what
                want = M.UNTOUCHED if n < 3 else (M.PLANE if n < 6 or order == 1 else None)
                if want is not None:
                    assert (got["status"] == want).all() and (ref["status"] == want).all(), what
                left_out += check(got, ref, cloud if q is None else q, 4.0, what)
                fewer_outputs_agree(ctx, capi, cloud, q, got, **fields)
    print("n %d: %d queries left out of the coordinate checks" % (n, left_out))


# ---- 3. exact cases
def lattice_plane(side, z):
    g = np.arange(side, dtype=np.float32)
    y, x = np.meshgrid(g, g, indexing="ij")
    return np.stack([x.ravel(), y.ravel(), np.full(side * side, z, np.float32)], axis=1)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("radius", [1.0, float(np.nextafter(np.sqrt(np.float32(2)), np.float32(2)))])
def test_a_lattice_plane_comes_back_bit_for_bit(ctx, capi, radius, mode):
    P = lattice_plane(9, 0.75)
    for order in (1, 2):
        got = run(ctx, capi, P, radius=radius, dist_mode=mode, order=order)
        ref = M.smooth(P, radius, mode, order=order)
        what = "lattice plane radius %g mode %d order %d" % (radius, mode, order)
        assert np.array_equal(got["neighbours"], ref["neighbours"]), what
        assert np.array_equal(bits(got["xyz"]), bits(P)), what                            # lambda0 = 0, every height 0, o = 0: exactly
        assert set(got["status"].tolist()) <= {M.QUADRATIC, M.PLANE} and (got["curvature"] == 0).all(), what
        assert (np.abs(got["normals"][:, 2]) == 1).all() and (got["normals"][:, :2] == 0).all(), what
        if order == 2 and radius > 1.0:
            assert (got["status"][ref["neighbours"] == 9] == M.QUADRATIC).all() and (got["status"][ref["neighbours"] < 6] == M.PLANE).all(), what
        else:
            assert (got["status"] == M.PLANE).all(), what


@pytest.mark.parametrize("mode", MODES)
def test_identical_and_collinear_points_stay_finite(ctx, capi, mode):
    same = np.tile(np.array([[1.5, -2.25, 3.0]], np.float32), (200, 1))
    got = run(ctx, capi, same, radius=1.0, dist_mode=mode)
    assert (got["neighbours"] == 200).all() and (got["status"] == M.PLANE).all() and np.array_equal(bits(got["xyz"]), bits(same))
    assert (got["curvature"] == 0).all() and np.isfinite(got["normals"]).all()
    line = np.stack([np.arange(70), 2.0 * np.arange(70), np.zeros(70)], axis=1).astype(np.float32)
    for radius in (1.0, 3.0, 400.0):                                                      # alone; with two neighbours; the whole line
        got = run(ctx, capi, line, radius=radius, dist_mode=mode)
        assert np.isfinite(got["xyz"]).all() and np.isfinite(got["normals"]).all() and np.isfinite(got["curvature"]).all(), radius
        assert set(got["status"].tolist()) <= {M.PLANE, M.UNTOUCHED}, radius
        assert np.array_equal(got["neighbours"], M.smooth(line, radius, mode)["neighbours"]), radius
        assert np.abs(got["xyz"].astype(np.float64) - line).max() <= 1e-4, radius          # a point of the line is its own foot
        if radius == 1.0:
            assert (got["status"] == M.UNTOUCHED).all() and np.array_equal(bits(got["xyz"]), bits(line)) and (bits(got["normals"]) == 0).all()


@pytest.mark.parametrize("mode", MODES)
def test_a_radius_that_holds_too_few_points_leaves_everything_untouched(ctx, capi, mode):
    cloud = clouds()["volume"][::5]
    queries = S.queries("volume")[:100]
    for q in (None, queries):
        for fields in (dict(radius=1e-3), dict(radius=1.6, min_neighbours=len(cloud) + 1)):
            got = run(ctx, capi, cloud, q, dist_mode=mode, **fields)
            src = cloud if q is None else q
            assert (got["status"] == M.UNTOUCHED).all() and np.array_equal(bits(got["xyz"]), bits(src)), fields
            assert (bits(got["normals"]) == 0).all() and (bits(got["curvature"]) == 0).all(), fields
            assert np.array_equal(got["neighbours"], M.smooth(cloud, fields["radius"], mode, queries=q)["neighbours"]), fields


# ---- 4. scale: beyond one grid layer per axis, and a case of the search suite's
@pytest.mark.parametrize("mode", MODES)
def test_a_surface_of_20000_points_on_sampled_rows(ctx, capi, mode):
    cloud, sample = wide_surface()
    got = run(ctx, capi, cloud, radius=0.9, dist_mode=mode)
    ref = M.smooth(cloud, 0.9, mode, only=sample)
    assert ref["neighbours"].mean() > 30 and (ref["status"] == M.QUADRATIC).mean() > 0.9
    check(got, ref, cloud, 0.9, "wide surface mode %d" % mode, only=sample)
    assert (got["status"] == M.QUADRATIC).mean() > 0.9


@pytest.mark.parametrize("mode", MODES)
def test_the_fine_grid_case_of_the_search_suite(ctx, capi, mode):
    queries, cloud = scale.cells_case(scale.FINE_POINTS, 0.0)                              # 66 000 points, 2 000 queries inside, on and outside the box
    sample = scale.sample_rows(len(queries), 192, 151)
    got = run(ctx, capi, cloud, queries, radius=0.5, dist_mode=mode)
    ref = M.smooth(cloud, 0.5, mode, queries=queries, only=sample, block=scale.reference_block(len(cloud)))
    assert 15 < ref["neighbours"].mean() < 60 and (ref["status"] == M.UNTOUCHED).any() and (ref["status"] == M.QUADRATIC).mean() > 0.5
    check(got, ref, queries, 0.5, "fine grid mode %d" % mode, only=sample)


# ---- 5. context hygiene
def test_a_loaded_icp_problem_survives(ctx, capi, golden):
    z = golden.npz("synth2k_clouds.npz")
    params = capi.icp_params(max_iterations=8)
    ctx.icp_load(z["before"], z["after"], params)
    ctx.icp_run(8)
    R0, t0, it0, err0, why0 = ctx.icp_result()
    ctx.icp_load(z["before"], z["after"], params)
    got = run(ctx, capi, clouds()["offset"], radius=0.9, dist_mode=K.DIST_FMA)
    assert (got["status"] == M.QUADRATIC).any()
    ctx.icp_run(8)
    R1, t1, it1, err1, why1 = ctx.icp_result()
    assert it0 > 0 and (it1, why1) == (it0, why0)
    assert np.array_equal(bits(R1), bits(R0)) and np.array_equal(bits(t1), bits(t0))
    assert np.float32(err1).tobytes() == np.float32(err0).tobytes()


def test_stage_times_sum_to_the_whole_call_while_profiling(ctx, capi):
    cloud = clouds()["surface"]
    run(ctx, capi, cloud, radius=0.9)                                  # (the buffers and the code object are there now)
    ctx.profile_enable(True)
    try:
        run(ctx, capi, cloud, radius=0.9)
        t = ctx.mls_smooth_times()
    finally:
        ctx.profile_enable(False)
    parts = sum(v for k, v in t.items() if k != "total")
    # every stage is drained, so the slots cover the call; the fit slot holds the launch's own event time, which the host's clock around
    # it can only exceed: the slots sum to the whole call from below, and to most of it
    assert all(v >= 0 for v in t.values()) and t["fit"] > 0 and t["total"] > 0, t
    assert 0.5 * t["total"] <= parts <= t["total"] * (1 + 1e-9), t


# ---- 6. refusals: nothing is written
def raw_call(ctx, capi, cloud, n, queries=None, nq=None, null_params=False, null_out=False, **fields):
    """mi_mls_smooth with every output prefilled with a sentinel -> (error code, message, outputs untouched?)"""
    rows = max(n if nq is None else nq, 1)
    xyz, normals, curvature = np.full(3 * rows, -7.5, np.float32), np.full(3 * rows, -7.5, np.float32), np.full(rows, -7.5, np.float32)
    neighbours, status = np.full(rows, -7, np.int32), np.full(rows, 7, np.uint8)
    p = capi.mls_params(**dict(dict(radius=0.9), **fields))
    rc = capi.mls_smooth_raw(ctx._h, None if cloud is None else cloud.ctypes.data, n, None if queries is None else queries.ctypes.data, n if nq is None else nq,
                             None if null_params else C.addressof(p), None if null_out else xyz.ctypes.data, normals.ctypes.data, curvature.ctypes.data,
                             neighbours.ctypes.data, status.ctypes.data)
    untouched = bool((xyz == -7.5).all() and (normals == -7.5).all() and (curvature == -7.5).all() and (neighbours == -7).all() and (status == 7).all())
    return rc, capi.lib().mi_last_error().decode(), untouched


def test_refusals_leave_the_outputs_untouched(ctx, capi):
    c = np.array(clouds()["surface"][:1000])
    q = np.array(S.queries("surface")[:100])
    nan, inf = float("nan"), float("inf")
    bad_args = [dict(cloud=None, n=1000), dict(cloud=c, n=1000, null_params=True), dict(cloud=c, n=1000, null_out=True),
                dict(cloud=c, n=0), dict(cloud=c, n=-1), dict(cloud=c, n=1000, queries=q, nq=0), dict(cloud=c, n=1000, nq=999),
                dict(cloud=c, n=1000, dist_mode=2), dict(cloud=c, n=1000, dist_mode=-1),
                dict(cloud=c, n=1000, min_neighbours=2), dict(cloud=c, n=1000, min_neighbours=-3),
                dict(cloud=c, n=1000, order=0), dict(cloud=c, n=1000, order=3)]
    bad_args += [dict(cloud=c, n=1000, radius=v) for v in (nan, inf, 0.0, -1.0, 1e20)]          # (1e20: the square is not finite)
    bad_args += [dict(cloud=c, n=1000, gauss_scale=v) for v in (nan, inf, -0.5)]
    for kw in bad_args:
        rc, msg, untouched = raw_call(ctx, capi, **kw)
        assert rc == capi.MI_ERR_INVALID_ARG and untouched and msg.startswith("mi_mls_smooth"), (kw, msg)
        named = [k for k in kw if k not in ("cloud", "n", "queries", "nq", "null_params", "null_out")]
        assert all(k in msg for k in named), (kw, msg)                  # the cause: the field's name
    # a bad point: its index -- the LOWEST one, of the cloud and of the queries
    for value in (np.nan, np.inf, -np.inf, 1.5e18, -1.5e18):
        bc = c.copy()
        bc[917, 2] = value
        bc[333, 0] = value
        rc, msg, untouched = raw_call(ctx, capi, bc, 1000)
        assert rc == capi.MI_ERR_INVALID_ARG and untouched and msg.startswith("mi_mls_smooth") and "cloud_xyz point 333 " in msg, (value, msg)
        bq = q.copy()
        bq[91, 1] = value
        bq[17, 2] = value
        rc, msg, untouched = raw_call(ctx, capi, c, 1000, queries=bq, nq=100)
        assert rc == capi.MI_ERR_INVALID_ARG and untouched and msg.startswith("mi_mls_smooth") and "query_xyz point 17 " in msg, (value, msg)
    with pytest.raises(capi.MiSlamError) as e:
        bc = c.copy()
        bc[5, 0] = np.nan
        ctx.mls_smooth(bc, capi.mls_params(radius=0.9))
    assert "cloud_xyz point 5 " in str(e.value)
    # and the context still works
    got = run(ctx, capi, clouds()["surface"], radius=0.9)
    check(got, S.reference("surface", False, K.DIST_CPU_ROUNDING, 2), clouds()["surface"], 0.9, "after the refusals")
