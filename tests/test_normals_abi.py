"""CPU suite: the normals entry points exist, a null context is refused without a device, and the restatement the GPU tests use as their
oracle (tests/normals_reference.py) gives answers worked by hand on the 3 x 3 x 3 integer lattice of tests/test_knn_abi.py."""
import ctypes as C

import numpy as np
import pytest

import knn_reference as K
import normals_reference as N


def test_library_exports_the_normals_entry_points(capi):
    lib = capi.lib()
    for name in ("mi_estimate_normals", "mi_estimate_normals_times"):
        assert hasattr(lib, name), name
        assert name in capi.EXPORTS, name
    assert lib.mi_abi_version() == 4          # additive: no signature of version 4 changed


def test_a_null_context_is_refused_without_a_device(capi):
    cloud = np.zeros((4, 3), np.float32)
    normals, curvature, count = np.full((4, 3), -7.5, np.float32), np.full(4, -7.5, np.float32), np.full(4, -7, np.int32)
    rc = capi.estimate_normals_raw(None, cloud.ctypes.data, 4, 2, capi.DIST_FMA, float("inf"), None, normals.ctypes.data, curvature.ctypes.data,
                                   count.ctypes.data)
    assert rc == capi.MI_ERR_INVALID_ARG and "null context" in capi.lib().mi_last_error().decode()
    assert capi.lib().mi_last_error().decode().startswith("mi_estimate_normals")
    assert (normals == -7.5).all() and (curvature == -7.5).all() and (count == -7).all()
    out = (C.c_double * 8)()
    f = capi.lib().mi_estimate_normals_times
    f.argtypes, f.restype = [C.c_void_p, C.c_void_p], C.c_int
    assert f(None, out) == capi.MI_ERR_INVALID_ARG


def lattice3():
    g = np.arange(3, dtype=np.float32)
    z, y, x = np.meshgrid(g, g, g, indexing="ij")
    return np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1)       # index = x + 3 y + 9 z


@pytest.mark.parametrize("mode", [K.DIST_CPU_ROUNDING, K.DIST_FMA])
def test_restatement_on_a_lattice_worked_by_hand(mode):
    L = lattice3()
    # the centre point with k = 6: itself and its six face neighbours; per axis the coordinates are 1 five times, 0 and 2 -> variance 2 / 7
    lam, normal, Cov, count = N.normals(L, 6, mode)
    assert count[13] == 6
    assert np.abs(Cov[13] - np.diag([2 / 7] * 3)).max() <= 1e-15
    assert np.abs(lam[13] - 2 / 7).max() <= 1e-15 and abs(N.curvature(lam)[13] - 1 / 3) <= 1e-15
    # the middle of a face with k = 5: four neighbours in the face and the centre point, all at distance 1.  Along the face's axis the
    # coordinates are one 1 and five equal ones (variance 5 / 36), along the other two 0, 2 and four 1s (variance 1 / 3): the normal
    # is the face's axis
    lam, normal, Cov, count = N.normals(L, 5, mode)
    for index, axis in ((4, 2), (22, 2), (10, 1), (16, 1), (12, 0), (14, 0)):
        assert count[index] == 5
        want = np.full(3, 1 / 3)
        want[axis] = 5 / 36
        assert np.abs(Cov[index] - np.diag(want)).max() <= 1e-15, index
        assert abs(abs(normal[index, axis]) - 1) <= 1e-15 and abs(lam[index, 0] - 5 / 36) <= 1e-15, index
        assert abs(N.curvature(lam)[index] - (5 / 36) / (5 / 36 + 2 / 3)) <= 1e-15
    # a corner with k = 2 has three neighbours at distance 1 and keeps the two of lowest index: three points, a plane through the corner
    lam, normal, Cov, count = N.normals(L, 2, mode)
    assert count[0] == 2 and abs(lam[0, 0]) <= 1e-16 and abs(abs(normal[0, 2]) - 1) <= 1e-15      # neighbours 1 (x) and 3 (y): normal z
    # fewer than three points, and the curvature rule where the trace is 0
    lam, normal, Cov, count = N.normals(L[:2], 4, mode)
    assert count.tolist() == [1, 1]
    assert N.curvature(np.zeros((1, 3)))[0] == 0.0 and N.curvature(np.array([[-1e-20, 1.0, 2.0]]))[0] == 0.0
