"""CPU suite: where the constant K of tests/test_gpu_mls.py's coordinate bound comes from, and that the main clouds are fit for it -- with the
restatement alone, before any device has been looked at.

The bound on a coordinate of out_xyz or out_normals is half an fp32 ulp of the reference value plus K (c + 8) 2^-53 radius / conditioning
(mls_reference.conditioning: the smallest pivot of the quadratic's scaled system; the eigenvalue gap over radius^2 where the plane
answered).  The restatement is run with every ball summed in ascending and in descending index order; the worst ratio of the spread between
the two, before the rounding to fp32, to the formula at K = 1 is measured here over every main case (three clouds, self mode and 500
queries of their own, order 1 and 2) and K is held to 4 x that ratio: the device's walk order is a third order.

Measured: 1.41 at the worst (volume cloud, self mode, order 2, a normal; out_xyz 0.97 on the offset cloud, where the fp64 spacing at 100
is itself 2.4 units of the formula).  K = 5.7.  No query of a main case is left out of the coordinate check (at most 1 % may be)."""
import numpy as np
import pytest

import knn_reference as K
import mls_cases as S
import mls_reference as M


@pytest.mark.parametrize("name", list(S.RADIUS))
def test_the_spread_between_two_summation_orders_sets_K(name):
    radius, worst = S.RADIUS[name], 0.0
    for separate in (False, True):
        for order in (1, 2):
            up = S.reference(name, separate, K.DIST_CPU_ROUNDING, order)
            down = S.reference(name, separate, K.DIST_CPU_ROUNDING, order, descending=True)
            assert np.array_equal(up["status"], down["status"]) and np.array_equal(up["neighbours"], down["neighbours"])
            pick = S.checked(up, radius)
            left_out = int(((up["status"] != M.UNTOUCHED) & ~pick).sum())
            near_floor = int(((up["pivot"] > M.PIVOT_MIN / 10) & (up["pivot"] < M.PIVOT_MIN * 10)).sum())
            unit = M.error_unit(up, radius)[pick]
            sign = np.where((up["normals64"] * down["normals64"]).sum(axis=1) >= 0, 1.0, -1.0)[:, None]
            rx = (np.abs(up["xyz64"] - down["xyz64"]).max(axis=1)[pick] / unit).max()
            rn = (np.abs(up["normals64"] - sign * down["normals64"]).max(axis=1)[pick] / unit).max()
            print("%s %s order %d: status counts %s, left out %d, within 10x of the pivot floor %d, spread / formula: xyz %.3f normals %.3f" % (
                name, "queries" if separate else "self", order, np.bincount(up["status"], minlength=3).tolist(), left_out, near_floor, rx, rn))
            assert left_out <= S.LEFT_OUT_SHARE * len(pick)
            assert near_floor == 0                                     # the status of every query is decided
            assert (up["status"] != M.UNTOUCHED).mean() > 0.9
            worst = max(worst, rx, rn)
    print("%s: worst spread / formula %.3f; K = %.1f" % (name, worst, S.K_BOUND))
    assert 4.0 * worst <= S.K_BOUND
