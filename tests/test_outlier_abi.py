"""CPU suite: the outlier-removal entry points exist, the argument errors that need no device are refused, the defaults are the
documented ones, and the restatement the GPU tests use as their oracle (tests/outlier_reference.py) gives the answers worked by hand
on the 3 x 3 x 3 integer lattice of tests/test_knn_abi.py."""
import ctypes as C

import numpy as np
import pytest

import knn_reference as K
import outlier_reference as R
from test_knn_abi import lattice3


def test_library_exports_the_outlier_entry_points(capi):
    lib = capi.lib()
    for name in ("mi_remove_outliers", "mi_remove_outliers_times", "mi_outlier_params_default"):
        assert hasattr(lib, name), name
        assert name in capi.EXPORTS, name
    assert lib.mi_abi_version() == 4          # additive: no signature of version 4 changed
    assert C.sizeof(capi.OutlierParams) == 12 * 4 and C.sizeof(capi.OutlierStats) == 3 * 8 + 8 + 4 * 4


def test_a_null_context_is_refused_without_a_device(capi):
    cloud = np.zeros((4, 3), np.float32)
    xyz, index, keep = np.full((4, 3), -7.5, np.float32), np.full(4, -7, np.int32), np.full(4, 7, np.uint8)
    mean_distance, neighbours = np.full(4, -7.5, np.float32), np.full(4, -7, np.int32)
    out_n, stats = C.c_int(-7), capi.OutlierStats(-7.5, -7.5, -7.5, -7)
    p = capi.outlier_params()
    rc = capi.remove_outliers_raw(None, cloud.ctypes.data, 4, C.addressof(p), xyz.ctypes.data, index.ctypes.data, C.addressof(out_n), keep.ctypes.data,
                                  mean_distance.ctypes.data, neighbours.ctypes.data, C.addressof(stats))
    msg = capi.lib().mi_last_error().decode()
    assert rc == capi.MI_ERR_INVALID_ARG and msg.startswith("mi_remove_outliers") and "null context" in msg
    assert (xyz == -7.5).all() and (index == -7).all() and (keep == 7).all() and (mean_distance == -7.5).all() and (neighbours == -7).all()
    assert out_n.value == -7 and (stats.mean, stats.stddev, stats.threshold, stats.kept) == (-7.5, -7.5, -7.5, -7)
    out = (C.c_double * 8)()
    f = capi.lib().mi_remove_outliers_times
    f.argtypes, f.restype = [C.c_void_p, C.c_void_p], C.c_int
    assert f(None, out) == capi.MI_ERR_INVALID_ARG


def test_defaults_are_the_documented_ones(capi):
    p = capi.outlier_params()
    assert (p.method, p.dist_mode, p.k, p.std_ratio) == (capi.OUTLIER_STATISTICAL, capi.DIST_CPU_ROUNDING, 16, 2.0)
    assert (p.radius, p.min_neighbours) == (0.0, 1) and list(p.reserved) == [0] * 6
    assert (capi.OUTLIER_STATISTICAL, capi.OUTLIER_RADIUS) == (0, 1)
    q = capi.outlier_params(method=capi.OUTLIER_RADIUS, radius=0.5, min_neighbours=3)
    assert (q.method, q.radius, q.min_neighbours, q.k) == (1, 0.5, 3, 16)
    with pytest.raises(AttributeError):
        capi.outlier_params(no_such_field=1)


@pytest.mark.parametrize("mode", [K.DIST_CPU_ROUNDING, K.DIST_FMA])
def test_restatement_on_a_lattice_worked_by_hand(mode):
    L = lattice3()                                                    # index = x + 3 y + 9 z
    on_boundary = ((L == 0) | (L == 2)).sum(axis=1)                   # 3: corner, 2: edge, 1: face, 0: the centre
    # radius 1: the face neighbours inside the lattice -- 3 at a corner, 4 on an edge, 5 on a face, 6 at the centre
    count, keep = R.radius(L, 1.0, 4, mode)
    assert count.tolist() == (6 - on_boundary).tolist() and sorted(set(count.tolist())) == [3, 4, 5, 6]
    assert (keep == (on_boundary < 3)).all() and int(keep.sum()) == 27 - 8
    count, keep = R.radius(L, 1.0, 6, mode)
    assert np.flatnonzero(keep).tolist() == [13]
    # the float below 1: no lattice point is that close to another
    assert (R.radius_counts(L, np.nextafter(np.float32(1), np.float32(0)), mode) == 0).all()
    # statistical, k = 3: every point has (at least) three neighbours at distance 1
    for ratio in (0.0, 1.0, 2.0):
        mu, count, (mean, stddev, threshold), keep = R.statistical(L, 3, mode, ratio)
        assert (mu == 1).all() and (count == 3).all() and (mean, stddev, threshold) == (1.0, 0.0, 1.0) and keep.all()
    # k = 6: the corners reach out to sqrt 2 three times, so they are the ones above a threshold of mean + 1 stddev
    mu, count, st, keep = R.statistical(L, 6, mode, 1.0)
    s2 = np.sqrt(2.0)
    assert mu[13] == 1 and mu[0] == (((3 + s2) + s2) + s2) / 6 and mu[1] == ((4 + s2) + s2) / 6 and mu[4] == (5 + s2) / 6
    assert (keep == (on_boundary < 3)).all()
    # a single point: no neighbour, score 0, kept by the statistical rule (0 <= 0) and removed by the radius rule
    one = L[:1]
    mu, count, st, keep = R.statistical(one, 8, mode, 0.0)
    assert mu.tolist() == [0.0] and count.tolist() == [0] and st == (0.0, 0.0, 0.0) and keep.tolist() == [True]
    assert R.radius(one, 1.0, 1, mode)[1].tolist() == [False]
