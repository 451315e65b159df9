"""GPU suite of mi_estimate_covariances against the float64 restatement of tests/gicp_reference.py, on the clouds, list sizes and shared
keys of tests/test_gpu_normals.py.

The bounds (none of them taken from what the device gives):
  count        equal to the restatement's and to mi_knn_search's own
  MI_COV_RAW   every entry equal, bit for bit, to the restatement's one-pass float64 covariance -- the nine sums added in the order of the
               keys, then S / c, Q / c - m m^T -- rounded once to fp32: additions, products and IEEE divisions only, no libm call
  MI_COV_PLANE where the neighbourhood's eigen-gap (lambda1 - lambda0) is at least 1e-3 of the trace (the normals suite's rule): every entry
               within 5e-7 of the restatement's I - (1 - eps) n n^T -- the entries move by 2 (1 - eps) |dn| <= 2 x 2e-7, the normals
               suite's bound on the direction, plus one fp32 rounding of an entry <= 1 (6e-8); at most 1 % of a cloud's points are left
               out, checked on the restatement's eigenvalues
  too few      count < 2: six zeros in both modes."""
import numpy as np
import pytest

import gicp_reference as G
import knn_reference as K
from test_gpu_normals import CLOUDS, MODES, bits, cloud_keys, clouds

pytestmark = pytest.mark.gpu

EPS = 1e-3


def check(ctx, capi, cloud, k, mode, what, idx=None, max_d2=np.inf, share=True):
    ref_raw = G.covariances(cloud, k, G.COV_RAW, EPS, mode, max_d2, idx=idx)
    ref_plane = G.covariances(cloud, k, G.COV_PLANE, EPS, mode, max_d2, idx=idx)
    raw, count = ctx.estimate_covariances(cloud, k, capi.COV_RAW, EPS, mode, max_d2, want_count=True)
    plane, count2 = ctx.estimate_covariances(cloud, k, capi.COV_PLANE, EPS, mode, max_d2, want_count=True)
    kcount = ctx.knn_search(None, cloud, k, mode, max_d2, want_d2=False, want_count=True)[1]
    assert np.array_equal(count, ref_raw["count"]) and np.array_equal(count2, count) and np.array_equal(count, kcount), what
    few = count < 2
    assert (raw[few] == 0).all() and (plane[few] == 0).all(), what
    assert np.array_equal(bits(raw), bits(ref_raw["cov"])), (what, np.abs(raw - ref_raw["cov"]).max())
    assert np.isfinite(plane).all(), what
    lam = ref_raw["lam"]
    trace = lam.sum(axis=1)
    gap_ok = ~few & (trace > 0) & ((lam[:, 1] - lam[:, 0]) >= 1e-3 * trace)
    err = np.abs(plane.astype(np.float64) - ref_plane["cov64"]).max(axis=1)
    print("%s: %d points, %d with too few neighbours, %d left out for their gap; plane entries off by %.3e at most" % (
        what, len(cloud), few.sum(), (~gap_ok & ~few).sum(), err[gap_ok].max(initial=0.0)))
    assert (err[gap_ok] <= 5e-7).all(), what
    if share:
        assert (~gap_ok & ~few).sum() <= 0.01 * len(cloud), what
    # wherever there is a covariance at all the device's is I - (1 - eps) n n^T of SOME unit n: trace 2 + eps, determinant eps
    M = G.full(plane[~few].astype(np.float64))
    assert (np.abs(np.trace(M, axis1=1, axis2=2) - (2 + EPS)) <= 1e-6).all() and (np.abs(np.linalg.det(M) - EPS) <= 1e-6).all(), what
    return raw, plane, count


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k", [4, 8, 16, 32])
@pytest.mark.parametrize("name", CLOUDS)
def test_covariances_of_the_normals_suites_clouds(ctx, capi, name, k, mode):
    cloud = clouds()[name]
    idx = K.unpack(cloud_keys(name, mode), k)[0]
    raw, plane, count = check(ctx, capi, cloud, k, mode, "%s k %d mode %d" % (name, k, mode), idx=idx)
    assert (count == k).all()
    # without the count the covariances are the same answer, and epsilon is not read in the raw mode
    assert np.array_equal(bits(ctx.estimate_covariances(cloud, k, capi.COV_RAW, 0.5, mode)), bits(raw))
    assert np.array_equal(bits(ctx.estimate_covariances(cloud, k, capi.COV_PLANE, EPS, mode)), bits(plane))


@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65])
def test_sizes_around_the_wave(ctx, capi, n):
    cloud = np.random.default_rng(1000 + n).uniform(-5, 5, (n, 3)).astype(np.float32)
    for mode in MODES:
        for k in (2, 8):
            raw, plane, count = check(ctx, capi, cloud, k, mode, "n %d k %d mode %d" % (n, k, mode), share=False)
            assert (count == min(k, n - 1)).all()
            if n < 3:
                assert (raw == 0).all() and (plane == 0).all()


@pytest.mark.parametrize("mode", MODES)
def test_distance_limit_and_too_few_neighbours(ctx, capi, mode):
    cloud, k = clouds()["volume"], 8
    limit = float(np.percentile(K.unpack(cloud_keys("volume", mode), k)[1][:, 1], 70))       # about 30 % of the points keep fewer than two
    raw, plane, count = check(ctx, capi, cloud, k, mode, "volume limit %g mode %d" % (limit, mode), max_d2=limit, share=False)
    assert 0.2 * len(cloud) < (count < 2).sum() < 0.4 * len(cloud) and (count >= 2).any()
    # a limit of 0 on a cloud with every point stored twice: the twin is the one neighbour, and two points make no covariance
    twins = np.concatenate([cloud[:500], cloud[:500]])
    for cov_mode in (capi.COV_RAW, capi.COV_PLANE):
        cov, count = ctx.estimate_covariances(twins, k, cov_mode, EPS, mode, 0.0, want_count=True)
        assert (count == 1).all() and (cov == 0).all()
    # epsilon at its ends
    check_ends = ctx.estimate_covariances(cloud, k, capi.COV_PLANE, 1.0, mode)
    assert np.array_equal(check_ends, np.tile(np.array([1, 0, 0, 1, 0, 1], np.float32), (len(cloud), 1)))
    flat = G.full(ctx.estimate_covariances(cloud, k, capi.COV_PLANE, 0.0, mode).astype(np.float64))
    assert (np.abs(np.linalg.det(flat)) <= 1e-6).all()


def test_refusals_leave_the_outputs_untouched(ctx, capi):
    c = np.array(clouds()["volume"][:1000])
    nan, inf = float("nan"), float("inf")

    def raw_call(cloud=c, n=1000, k=8, mode=0, max_d2=inf, cov_mode=capi.COV_PLANE, epsilon=1e-3, null_cov=False):
        cov, count = np.full(6 * max(n, 1), -7.5, np.float32), np.full(max(n, 1), -7, np.int32)
        rc = capi.estimate_covariances_raw(ctx._h, None if cloud is None else cloud.ctypes.data, n, k, mode, float(max_d2), cov_mode, epsilon,
                                           None if null_cov else cov.ctypes.data, count.ctypes.data)
        return rc, capi.lib().mi_last_error().decode(), bool((cov == -7.5).all() and (count == -7).all())

    bad_args = [dict(k=1), dict(k=33), dict(k=0), dict(mode=2), dict(mode=-1), dict(max_d2=nan), dict(max_d2=-1.0), dict(cloud=None), dict(null_cov=True),
                dict(n=0), dict(n=-1), dict(cov_mode=2), dict(cov_mode=-1), dict(epsilon=nan), dict(epsilon=-1e-3), dict(epsilon=1.5), dict(epsilon=inf)]
    for kw in bad_args:
        rc, msg, untouched = raw_call(**kw)
        assert rc == capi.MI_ERR_INVALID_ARG and untouched and msg.startswith("mi_estimate_covariances"), (kw, msg)
    assert raw_call(cov_mode=capi.COV_RAW, epsilon=nan)[0] == 0                          # epsilon is ignored in the raw mode
    for value in (nan, inf, -inf, 1.5e18):
        bc = c.copy()
        bc[917, 2] = value
        bc[333, 0] = value
        rc, msg, untouched = raw_call(cloud=bc)
        assert rc == capi.MI_ERR_INVALID_ARG and untouched and msg.startswith("mi_estimate_covariances") and "cloud_xyz point 333 " in msg, (value, msg)
    with pytest.raises(capi.MiSlamError):
        ctx.estimate_covariances(c, 8, 7)
    assert np.isfinite(ctx.estimate_covariances(c, 8)).all()                             # and the context still works
