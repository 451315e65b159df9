"""GPU suite of mi_estimate_normals against the float64 restatement of tests/normals_reference.py.  The O(n^2) part of the restatement,
the sorted keys of tests/knn_reference.py in self mode, is built once per cloud and arithmetic (lru_cache) and shared by every k.

The bounds (none of them taken from what the device gives):
  Rayleigh quotient   n^T C_ref n / n^T n - lambda0_ref <= 1e-12 trace(C_ref), the device's fp32 normal taken to float64.  The
                      reference's own eigenvector rounded to fp32 stays below 1.5e-15: the rounding's angle of 5e-8 enters squared.
                      A wrong eigenvector at a gap of 1e-3 is out by at least 1e-3: three orders of room above, nine below.
  unit length         | |n| - 1 | <= 2e-7
  direction           where (lambda1 - lambda0) / trace >= 1e-3: min(|n - n_ref|, |n + n_ref|) <= 2e-7 -- fp32 rounding of three
                      components <= 1 gives sqrt(3) 2^-25 = 5.2e-8, the fp64 solve at that gap about 1e-11; a margin of about 4
  curvature           | sigma - sigma_ref | <= 6e-8, two fp32 ulps at 1/3; exactly 0 where the rule says 0
  count               equal."""
import functools

import numpy as np
import pytest

import knn_reference as K
import normals_reference as N

pytestmark = pytest.mark.gpu

MODES = (K.DIST_CPU_ROUNDING, K.DIST_FMA)
CLOUDS = ("sphere", "sphere_offset", "volume", "plane_noise")
VIEWPOINTS = {"sphere": (0.0, 0.0, 0.0), "plane_noise": (0.0, 0.0, 100.0), "volume": (0.5, -1.0, 2.0)}


def frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def clouds():
    rng = np.random.default_rng(71)
    n = 2000

    def shell():
        d = rng.normal(size=(n, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        return d * (1 + 0.01 * rng.normal(size=n))[:, None]

    out = {"sphere": shell(), "sphere_offset": shell() + np.array([100.0, -50.0, 25.0]), "volume": rng.uniform(-5, 5, (n, 3))}
    xy = rng.uniform(-5, 5, (n, 2))
    out["plane_noise"] = np.concatenate([xy, (0.3 * xy[:, 0] - 0.2 * xy[:, 1] + 0.02 * rng.normal(size=n))[:, None]], axis=1)
    return {name: frozen(np.ascontiguousarray(c, np.float32)) for name, c in out.items()}


@functools.lru_cache(maxsize=None)
def cloud_keys(name, mode):
    return frozen(K.sorted_keys(None, clouds()[name], mode))


@functools.lru_cache(maxsize=None)
def reference(name, k, mode):
    return N.from_neighbours(clouds()[name], K.unpack(cloud_keys(name, mode), k)[0])


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(got, want):
    return all(np.array_equal(bits(g), bits(w)) for g, w in zip(got, want))


def check(ref, got, what, share=True):
    """Checks 1 - 5 of one device answer (normals, curvature, count) against the restatement's (lambda, normal, C, count)."""
    lam, n_ref, C, count_ref = ref
    normals, curvature, count = got
    assert np.isfinite(normals).all() and np.isfinite(curvature).all(), what
    assert np.array_equal(count, count_ref), what                                                      # 5
    valid = count_ref >= 2
    assert (normals[~valid] == 0).all() and (curvature[~valid] == 0).all(), what                       # too few points
    if not valid.any():
        return
    lam, n_ref, C, n64, sigma = lam[valid], n_ref[valid], C[valid], normals[valid].astype(np.float64), curvature[valid].astype(np.float64)
    trace = np.trace(C, axis1=1, axis2=2)
    length2 = (n64 * n64).sum(axis=1)
    excess = np.einsum("ni,nij,nj->n", n64, C, n64) / length2 - lam[:, 0]                              # 1
    length_error = np.abs(np.sqrt(length2) - 1)                                                        # 2
    print("%s: %d valid points; Rayleigh excess / trace %.3e, | |n| - 1 | %.3e" % (
        what, valid.sum(), (excess[trace > 0] / trace[trace > 0]).max(initial=0.0), length_error.max()), end="")
    assert (excess <= 1e-12 * trace).all(), what
    assert (length_error <= 2e-7).all(), what
    gap_ok = (lam[:, 1] - lam[:, 0]) >= 1e-3 * trace                                                   # 3
    gap_ok &= trace > 0
    d = np.minimum(np.linalg.norm(n64 - n_ref, axis=1), np.linalg.norm(n64 + n_ref, axis=1))
    sigma_ref = N.curvature(lam)
    print("; direction %.3e over %d points (%d left out); curvature %.3e" % (
        d[gap_ok].max(initial=0.0), gap_ok.sum(), (~gap_ok).sum(), np.abs(sigma - sigma_ref).max()))
    assert (d[gap_ok] <= 2e-7).all(), what
    if share:
        assert (~gap_ok).sum() <= 0.01 * len(gap_ok), what
    assert (np.abs(sigma - sigma_ref) <= 6e-8).all(), what                                             # 4
    assert (sigma[lam.sum(axis=1) <= 0] == 0).all(), what


def call(ctx, cloud, k, mode, viewpoint=None, max_d2=np.inf):
    return ctx.estimate_normals(cloud, k, viewpoint, mode, max_d2, want_curvature=True, want_count=True)


# ---- 1 - 5. every cloud, every list size, both arithmetics
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k", [4, 8, 16, 32])
@pytest.mark.parametrize("name", CLOUDS)
def test_normals_curvature_and_count(ctx, name, k, mode):
    got = call(ctx, clouds()[name], k, mode)
    check(reference(name, k, mode), got, "%s k %d mode %d" % (name, k, mode))
    # the normals alone are the same answer
    assert np.array_equal(bits(ctx.estimate_normals(clouds()[name], k, None, mode)), bits(got[0]))


# ---- 6. the viewpoint
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", sorted(VIEWPOINTS))
def test_viewpoint_turns_the_normals(ctx, name, mode):
    cloud, k = clouds()[name], 8
    v = np.array(VIEWPOINTS[name], np.float32)
    free = call(ctx, cloud, k, mode)
    got = call(ctx, cloud, k, mode, viewpoint=v)
    lam, n_ref, C, count_ref = reference(name, k, mode)
    assert (count_ref >= 2).all()
    to_view = v.astype(np.float64)[None, :] - cloud.astype(np.float64)
    towards = (got[0].astype(np.float64) * to_view).sum(axis=1)
    assert (towards >= 0).all(), (name, towards.min())
    # the unoriented call's normals up to sign, bit for bit in magnitude; curvature and count untouched
    assert np.array_equal(bits(got[0]) & 0x7fffffff, bits(free[0]) & 0x7fffffff)
    assert ((got[0] == free[0]).all(axis=1) | (got[0] == -free[0]).all(axis=1)).all()
    assert same_bits(got[1:], free[1:])
    if name == "sphere":
        assert ((got[0].astype(np.float64) * cloud.astype(np.float64)).sum(axis=1) < 0).all()
    # the sign against the restatement's, where that is not a matter of rounding
    ref_towards = (n_ref * to_view).sum(axis=1)
    clear = np.abs(ref_towards) >= 1e-6 * np.linalg.norm(to_view, axis=1)
    oriented_ref = n_ref * np.sign(ref_towards)[:, None]
    assert clear.sum() > 0.9 * len(cloud) and ((got[0].astype(np.float64) * oriented_ref).sum(axis=1)[clear] > 0).all()
    check((lam, n_ref, C, count_ref), got, "%s viewpoint mode %d" % (name, mode))


# ---- 7. the distance limit: the hybrid k-and-radius neighbourhood
@pytest.mark.parametrize("mode", MODES)
def test_distance_limit(ctx, mode):
    cloud, k = clouds()["volume"], 8
    limit = float(np.median(K.unpack(cloud_keys("volume", mode), k)[1][:, k - 1]))              # half the points are cut short
    ref = N.normals(cloud, k, mode, limit)
    got = call(ctx, cloud, k, mode, max_d2=limit)
    assert 0 < (ref[3] < k).sum() < len(cloud)
    check(ref, got, "volume limit %g mode %d" % (limit, mode))
    # a limit of 0 on a cloud with every point stored twice: the twin is the one neighbour, and two points make no normal
    twins = np.concatenate([cloud[:500], cloud[:500]])
    normals, curvature, count = call(ctx, twins, k, mode, max_d2=0.0)
    assert (count == 1).all() and (normals == 0).all() and (curvature == 0).all()


# ---- 8. the smallest shapes: around the one-wave workgroup's edge, every list size at its edge and one past it
SMALL = [(1, 2), (2, 2), (3, 2), (2, 8), (3, 8), (8, 8), (9, 8), (9, 9), (10, 9), (16, 16), (17, 16), (17, 17), (18, 17), (32, 32), (33, 32),
         (63, 8), (64, 8), (65, 8), (63, 17), (64, 32), (65, 32), (65, 2)]


@pytest.mark.parametrize("n,k", SMALL)
def test_smallest_shapes(ctx, n, k):
    rng = np.random.default_rng(1000 * n + k)
    cloud = rng.uniform(-5, 5, (n, 3)).astype(np.float32)
    for mode in MODES:
        ref = N.normals(cloud, k, mode)
        assert (ref[3] == min(k, n - 1)).all()
        check(ref, call(ctx, cloud, k, mode), "n %d k %d mode %d" % (n, k, mode), share=False)


# ---- 9. awkward clouds (those of tests/test_gpu_knn.py, built here)
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
def test_awkward_clouds(ctx, kind):
    cloud = awkward_cloud(kind)
    for mode in MODES:
        lam, n_ref, C, count_ref = N.normals(cloud, 8, mode)
        normals, curvature, count = call(ctx, cloud, 8, mode)
        assert np.isfinite(normals).all() and np.isfinite(curvature).all() and np.array_equal(count, count_ref)
        n64 = normals.astype(np.float64)
        length2 = (n64 * n64).sum(axis=1)
        assert (np.abs(np.sqrt(length2) - 1) <= 2e-7).all()                 # (count = 8 everywhere: finite and of unit length)
        trace = np.trace(C, axis1=1, axis2=2)
        excess = np.einsum("ni,nij,nj->n", n64, C, n64) / length2 - lam[:, 0]
        some = trace > 0
        print("%s mode %d: Rayleigh excess / trace %.3e over %d points" % (kind, mode, (excess[some] / trace[some]).max(initial=0.0), some.sum()))
        assert (excess[some] <= 1e-12 * trace[some]).all()
        if kind == "coplanar":
            assert (np.abs(normals[:, 2]) >= 1 - 1e-6).all() and (curvature <= 1e-12).all()
        if kind == "identical":
            assert (curvature == 0).all()


# ---- 10. every cell regime gives the default's bits
@pytest.mark.parametrize("ppc", ["0.25", "8", "1e9"])
def test_cell_regimes_give_the_same_bits(ctx, capi, monkeypatch, ppc):
    cloud = clouds()["volume"]
    want = {mode: call(ctx, cloud, 16, mode) for mode in MODES}
    monkeypatch.setenv("MISLAM_KNN_POINTS_PER_CELL", ppc)
    with capi.Context(0) as c2:
        for mode in MODES:
            assert same_bits(call(c2, cloud, 16, mode), want[mode]), (ppc, mode)


# ---- 11. context hygiene
def test_a_loaded_icp_problem_survives_and_calls_do_not_leak_into_each_other(ctx, capi, golden):
    z = golden.npz("synth2k_clouds.npz")
    params = capi.icp_params(max_iterations=8)
    ctx.icp_load(z["before"], z["after"], params)
    ctx.icp_run(8)
    R0, t0, it0, err0, why0 = ctx.icp_result()
    ctx.icp_load(z["before"], z["after"], params)
    cloud = clouds()["sphere_offset"]
    knn_first = ctx.knn_search(None, cloud, 8, K.DIST_FMA, want_count=True)
    first = call(ctx, cloud, 8, K.DIST_FMA)
    ctx.icp_run(8)
    R1, t1, it1, err1, why1 = ctx.icp_result()
    assert it0 > 0 and (it1, why1) == (it0, why0)
    assert np.array_equal(bits(R1), bits(R0)) and np.array_equal(bits(t1), bits(t0))
    assert np.float32(err1).tobytes() == np.float32(err0).tobytes()
    # calls of other sizes (and k, arithmetic, viewpoint, limit) in between leave nothing behind
    call(ctx, clouds()["volume"][:65], 32, K.DIST_CPU_ROUNDING, viewpoint=(1.0, 2.0, 3.0))
    ctx.estimate_normals(z["after"], 3, None, K.DIST_CPU_ROUNDING, 1.0)
    assert same_bits(call(ctx, cloud, 8, K.DIST_FMA), first)
    assert same_bits(ctx.knn_search(None, cloud, 8, K.DIST_FMA, want_count=True), knn_first)


# ---- 12. refusals: nothing is written
def raw_call(ctx, capi, cloud, n, k, mode=0, max_d2=np.inf, viewpoint=None, null_normals=False):
    """mi_estimate_normals with every output prefilled with a sentinel -> (error code, message, outputs untouched?)"""
    rows = max(n, 1)
    normals, curvature, count = np.full(3 * rows, -7.5, np.float32), np.full(rows, -7.5, np.float32), np.full(rows, -7, np.int32)
    view = None if viewpoint is None else np.array(viewpoint, np.float32)
    rc = capi.estimate_normals_raw(ctx._h, None if cloud is None else cloud.ctypes.data, n, k, mode, float(max_d2), None if view is None else view.ctypes.data,
                                   None if null_normals else normals.ctypes.data, curvature.ctypes.data, count.ctypes.data)
    return rc, capi.lib().mi_last_error().decode(), bool((normals == -7.5).all() and (curvature == -7.5).all() and (count == -7).all())


def test_refusals_leave_the_outputs_untouched(ctx, capi):
    c = np.array(clouds()["volume"][:1000])
    bad_args = [
        dict(cloud=c, n=1000, k=1), dict(cloud=c, n=1000, k=33), dict(cloud=c, n=1000, k=0), dict(cloud=c, n=1000, k=-1),
        dict(cloud=c, n=1000, k=8, mode=2), dict(cloud=c, n=1000, k=8, mode=-1),
        dict(cloud=c, n=1000, k=8, max_d2=float("nan")), dict(cloud=c, n=1000, k=8, max_d2=-1.0), dict(cloud=c, n=1000, k=8, max_d2=float("-inf")),
        dict(cloud=None, n=1000, k=8), dict(cloud=c, n=1000, k=8, null_normals=True),
        dict(cloud=c, n=0, k=8), dict(cloud=c, n=-1, k=8),
        dict(cloud=c, n=1000, k=8, viewpoint=(np.nan, 0, 0)), dict(cloud=c, n=1000, k=8, viewpoint=(0, 0, np.inf)),
    ]
    for kw in bad_args:
        rc, msg, untouched = raw_call(ctx, capi, **kw)
        assert rc == capi.MI_ERR_INVALID_ARG and untouched and msg.startswith("mi_estimate_normals"), (kw, msg)
    # a bad point: its index -- the LOWEST one, in mi_knn_search's wording
    for value in (np.nan, np.inf, -np.inf, 1.5e18, -1.5e18):
        bc = c.copy()
        bc[917, 2] = value
        bc[333, 0] = value
        rc, msg, untouched = raw_call(ctx, capi, bc, 1000, 8)
        assert rc == capi.MI_ERR_INVALID_ARG and untouched and msg.startswith("mi_estimate_normals") and "cloud_xyz point 333 " in msg, (value, msg)
        rc2 = capi.knn_search_raw(ctx._h, None, 1000, bc.ctypes.data, 1000, 8, 0, float("inf"), np.empty(8000, np.int32).ctypes.data, None, None)
        assert rc2 == capi.MI_ERR_INVALID_ARG and capi.lib().mi_last_error().decode() == msg.replace("mi_estimate_normals", "mi_knn_search")
    with pytest.raises(capi.MiSlamError) as e:
        bc = c.copy()
        bc[5, 0] = np.nan
        ctx.estimate_normals(bc, 8)
    assert "cloud_xyz point 5 " in str(e.value)
    # the largest coordinates the call accepts: everything stays finite
    big = np.array([[1e18, -1e18, 1e18], [-1e18, 1e18, -1e18], [0, 0, 0], [1e18, 1e18, 0]], np.float32)
    normals, curvature, count = call(ctx, big, 3, K.DIST_FMA)
    assert (count == 3).all() and np.isfinite(normals).all() and np.isfinite(curvature).all()
    check(reference("volume", 8, K.DIST_CPU_ROUNDING), call(ctx, clouds()["volume"], 8, K.DIST_CPU_ROUNDING), "after the refusals")   # and the context still works
