"""The range pass every cloud-taking call opens with (csrc/cloud_range.hpp), through mi_selftest_cloud_range: per-axis minimum and maximum
over the usable points and the lowest refused index.  Every result is one of the inputs, so every comparison is exact: the float32 bits
of numpy's min / max over the usable points, and the index itself.

Sizes: 1, 63, 255, 256, 257 (a lane short of / exactly / one past a block) and 65 537 = 256 blocks x 256 lanes + 1: one lane takes a second
trip of the stride loop (index 65 536) and the finish folds a full 256 rows."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NO_POINT = 0x7FFFFFFF
SIZES = [1, 63, 255, 256, 257, 65537]
INF = np.float32(np.inf)


def cloud(n, seed=0):
    return np.random.default_rng(1000 * seed + n).uniform(-5.0, 5.0, (n, 3)).astype(np.float32)       # (no zeros: see the signed-zero test)


def usable(p, check):
    if check == 0:
        return np.ones(len(p), bool)
    if check == 1:
        return np.isfinite(p).all(axis=1)
    with np.errstate(invalid="ignore"):
        return (np.abs(p) <= np.float32(1e18)).all(axis=1)             # (false for NaN and the infinities)


def expected(p, check):
    ok = usable(p, check)
    q = p[ok]
    lo = q.min(axis=0) if len(q) else np.full(3, INF)
    hi = q.max(axis=0) if len(q) else np.full(3, -INF)
    bad = int(np.flatnonzero(~ok)[0]) if not ok.all() else NO_POINT
    return np.concatenate([lo, hi]).astype(np.float32), bad


def check_against_numpy(ctx, p, check):
    lo_hi, bad = ctx.selftest_cloud_range(p, check)
    want, want_bad = expected(p, check)
    print("n", len(p), "check", check, "got", lo_hi, bad, "want", want, want_bad)
    assert np.array_equal(lo_hi.view(np.uint32), want.view(np.uint32))
    assert bad == want_bad


@pytest.mark.parametrize("check", [0, 1, 2])
@pytest.mark.parametrize("n", SIZES)
def test_clean_cloud_matches_numpy(ctx, n, check):
    p = cloud(n)
    check_against_numpy(ctx, p, check)
    assert ctx.selftest_cloud_range(p, check)[1] == NO_POINT


@pytest.mark.parametrize("check", [1, 2])
@pytest.mark.parametrize("n,at", [(257, 0), (257, 256), (65537, 0), (65537, 65536), (65537, 40000)])
def test_one_refused_point_is_reported_and_contributes_nothing(ctx, n, at, check):
    p = cloud(n, 1)
    p[at] = (np.nan, 1e6, -1e6)           # its other coordinates would be the extremes
    lo_hi, bad = ctx.selftest_cloud_range(p, check)
    assert bad == at and np.abs(lo_hi).max() <= 5.0
    check_against_numpy(ctx, p, check)


@pytest.mark.parametrize("check", [1, 2])
@pytest.mark.parametrize("first,second", [(0, 65536), (300, 65536), (255, 256), (65535, 65536)])
def test_of_two_refused_points_the_lower_index_is_reported(ctx, first, second, check):
    p = cloud(65537, 2)
    p[second] = (np.inf, 0.5, 0.5)
    p[first] = (0.5, 0.5, np.nan)
    check_against_numpy(ctx, p, check)
    assert ctx.selftest_cloud_range(p, check)[1] == first
    assert ctx.selftest_cloud_range(p[::-1], check)[1] == 65536 - second


def test_what_each_check_refuses(ctx):
    for n in (5, 65537):
        for value, refused_by_2, refused_by_1 in ((2e18, True, False), (-2e18, True, False), (1e18, False, False), (-1e18, False, False),
                                                  (np.inf, True, True), (-np.inf, True, True), (np.nan, True, True)):
            for axis in (range(3) if n == 5 else (1,)):
                p = cloud(n, 3)
                p[n - 2, axis] = value
                assert (ctx.selftest_cloud_range(p, 2)[1] == n - 2) == refused_by_2, (value, axis)
                assert (ctx.selftest_cloud_range(p, 1)[1] == n - 2) == refused_by_1, (value, axis)
                assert ctx.selftest_cloud_range(p, 0)[1] == NO_POINT
                for check in (0, 1, 2):
                    if check == 0 and np.isnan(value):
                        continue                      # (the NaN test below)
                    check_against_numpy(ctx, p, check)
    # a coordinate of 2e18 that check 1 lets through IS the maximum
    p = cloud(300, 4)
    p[7, 1] = 2e18
    assert ctx.selftest_cloud_range(p, 1)[0][4] == np.float32(2e18)


@pytest.mark.parametrize("check", [1, 2])
@pytest.mark.parametrize("n", [1, 300, 65537])
def test_every_point_refused(ctx, n, check):
    p = cloud(n, 5)
    p[:, n % 3] = np.nan
    lo_hi, bad = ctx.selftest_cloud_range(p, check)
    assert np.array_equal(lo_hi, np.array([INF, INF, INF, -INF, -INF, -INF], np.float32)) and bad == 0


@pytest.mark.parametrize("n", [63, 257, 65537])
def test_without_a_predicate_nan_coordinates_are_ignored(ctx, n):
    rng = np.random.default_rng(n)
    p = cloud(n, 6)
    p[rng.random((n, 3)) < 0.3] = np.nan
    p[0] = (np.nan, 1.0, np.nan)
    p[n - 1] = (np.nan, np.nan, 2.0)
    p[n // 2] = (0.25, 0.25, 0.25)         # (no axis is NaN throughout)
    # the extremes themselves sit beside NaNs in their rows
    p[n // 3] = (-7.0, np.nan, 7.0)
    lo_hi, bad = ctx.selftest_cloud_range(p, 0)
    want = np.concatenate([np.nanmin(p, axis=0), np.nanmax(p, axis=0)]).astype(np.float32)
    print("got", lo_hi, "want", want)
    assert np.array_equal(lo_hi.view(np.uint32), want.view(np.uint32)) and bad == NO_POINT
    assert lo_hi[0] == -7.0 and lo_hi[5] == 7.0


@pytest.mark.parametrize("check", [0, 1, 2])
@pytest.mark.parametrize("n", [2, 257, 65537])
def test_a_zero_extreme_has_one_sign_whatever_the_order(ctx, n, check):
    # x >= 0 with both zeros among the minima, y <= 0 with both zeros among the maxima, z nothing but zeros of both signs
    rng = np.random.default_rng(n)
    p = np.abs(cloud(n, 7))
    p[:, 1] *= -1
    p[:, 2] = np.where(rng.random(n) < 0.5, np.float32(0.0), np.float32(-0.0))
    for i, z in ((0, 0.0), (n - 1, -0.0), (n // 2, 0.0), (n // 3, -0.0)):
        p[i] = (z, -z, z)
    p[0, 2], p[n - 1, 2] = 0.0, -0.0
    a, bad_a = ctx.selftest_cloud_range(p, check)
    b, bad_b = ctx.selftest_cloud_range(p[::-1], check)
    print("forward", a, np.signbit(a), "reversed", b, np.signbit(b))
    assert bad_a == NO_POINT and bad_b == NO_POINT
    assert a[0] == 0 and a[4] == 0 and a[2] == 0 and a[5] == 0
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_bad_arguments_are_refused(ctx, capi):
    p = cloud(4)
    with pytest.raises(capi.MiSlamError):
        ctx.selftest_cloud_range(p, 3)
    with pytest.raises(capi.MiSlamError):
        ctx.selftest_cloud_range(p[:0], 0)
