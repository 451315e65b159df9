"""CPU suite: the point-to-plane entry points exist with the stated defaults, a null context is refused without a device and with the outputs
untouched, and the restatement the GPU tests use as their oracle (tests/plane_reference.py) gives the answers worked by hand on a
3 x 3 lattice plane."""
import ctypes as C

import numpy as np
import pytest

import knn_reference as K
import plane_reference as P


def test_library_exports_the_plane_entry_points(capi):
    lib = capi.lib()
    for name in ("mi_plane_params_default", "mi_icp_plane_register", "mi_plane_system", "mi_icp_plane_times"):
        assert hasattr(lib, name), name
        assert name in capi.EXPORTS, name
    assert lib.mi_abi_version() == 4          # additive: no signature of version 4 changed
    assert capi.STOP_DEGENERATE == 7 == P.STOP_DEGENERATE


def test_defaults_are_as_stated(capi):
    assert C.sizeof(capi.PlaneParams) == 16 * 4
    p = capi.plane_params()
    assert (p.eps_rotation, p.eps_translation) == (np.float32(1e-6), np.float32(1e-6))
    assert (p.max_iterations, p.max_distance_squared, p.dist_mode, p.sync_every, p.verbose) == (50, float("inf"), capi.DIST_CPU_ROUNDING, 0, 0)
    assert list(p.reserved) == [0] * 9
    assert capi.plane_params(max_iterations=3, sync_every=2).max_iterations == 3
    with pytest.raises(AttributeError):
        capi.plane_params(no_such_field=1)


def test_a_null_context_is_refused_without_a_device(capi):
    cloud, normals = np.zeros((4, 3), np.float32), np.tile(np.array([0, 0, 1], np.float32), (4, 1))
    T, it, err, why = np.full(16, -7.5, np.float32), C.c_int(-7), C.c_float(-7.5), C.c_int(-7)
    p = capi.plane_params()
    rc = capi.icp_plane_register_raw(None, cloud.ctypes.data, 4, cloud.ctypes.data, normals.ctypes.data, 4, C.addressof(p), None, T.ctypes.data,
                                     C.addressof(it), C.addressof(err), C.addressof(why))
    assert rc == capi.MI_ERR_INVALID_ARG and "null context" in capi.lib().mi_last_error().decode()
    assert capi.lib().mi_last_error().decode().startswith("mi_icp_plane_register")
    assert (T == -7.5).all() and it.value == -7 and err.value == -7.5 and why.value == -7
    sums, centre, idx = np.full(32, -7.5), np.full(3, -7.5, np.float32), np.full(4, -7, np.int32)
    rc = capi.plane_system_raw(None, cloud.ctypes.data, 4, cloud.ctypes.data, normals.ctypes.data, 4, None, capi.DIST_FMA, float("inf"), sums.ctypes.data,
                               centre.ctypes.data, idx.ctypes.data)
    assert rc == capi.MI_ERR_INVALID_ARG and capi.lib().mi_last_error().decode().startswith("mi_plane_system: null context")
    assert (sums == -7.5).all() and (centre == -7.5).all() and (idx == -7).all()
    out = (C.c_double * 8)()
    f = capi.lib().mi_icp_plane_times
    f.argtypes, f.restype = [C.c_void_p, C.c_void_p], C.c_int
    assert f(None, out) == capi.MI_ERR_INVALID_ARG


def lattice_plane():
    g = np.arange(3, dtype=np.float32)
    y, x = np.meshgrid(g, g, indexing="ij")
    return np.stack([x.ravel(), y.ravel(), np.zeros(9, np.float32)], axis=1)       # index = x + 3 y, z = 0


@pytest.mark.parametrize("mode", [K.DIST_CPU_ROUNDING, K.DIST_FMA])
def test_restatement_on_a_lattice_plane_worked_by_hand(mode):
    fixed = lattice_plane()
    normals = np.tile(np.array([0, 0, 1], np.float32), (9, 1))
    moving = fixed + np.array([0, 0, 0.5], np.float32)
    sy = P.system(moving, fixed, normals, dist_mode=mode)
    # every moving point sits 0.5 above its own lattice point: that is its match, r = 0.5, d2 = 0.25
    assert sy["idx"].tolist() == list(range(9)) and sy["centre"].tolist() == [1.0, 1.0, 0.0]
    s = sy["sums"]
    assert s[29] == 9 and s[27] == 9 * 0.25 and s[28] == 9 * 0.25 and (s[30:] == 0).all()
    # J = (p_y, -p_x, 0, 0, 0, 1) with p = q - c0, p_x and p_y each -1, 0, 1 three times: sum p_y^2 = sum p_x^2 = 6, every mixed sum 0
    A, g = P.unpack_system(s)
    want = np.zeros((6, 6))
    want[0, 0] = want[1, 1] = 6.0
    want[5, 5] = 9.0
    assert np.array_equal(A, want)
    assert np.array_equal(g, [0, 0, 0, 0, 0, 4.5])                               # sum J r: only the z translation sees the lift
    # rotation about z and translation along x and y move no point off the plane: three zero diagonal entries, degenerate, pose untouched
    st = P.step(moving, fixed, normals, np.eye(3), np.zeros(3), mode)
    assert st["stop"] == P.STOP_DEGENERATE and np.array_equal(st["R"], np.eye(3)) and np.array_equal(st["t"], np.zeros(3))
    assert st["error"] == np.float32(0.25)
    out = P.register(moving, fixed, normals, dist_mode=mode)
    assert out["stop"] == P.STOP_DEGENERATE and out["iterations"] == 0 and out["error"] == np.float32(0.25)
    # a zero normal is no pair, a limit below the lift leaves none, and fewer than six pairs is STOP_NO_PAIRS
    holes = normals.copy()
    holes[[0, 4]] = 0
    sy = P.system(moving, fixed, holes, dist_mode=mode)
    assert sy["idx"].tolist() == [-1, 1, 2, 3, -1, 5, 6, 7, 8] and sy["sums"][29] == 7
    assert (P.system(moving, fixed, normals, dist_mode=mode, max_d2=0.2)["idx"] == -1).all()
    assert P.register(moving, fixed, normals, dist_mode=mode, max_d2=0.2)["stop"] == P.STOP_NO_PAIRS
    assert P.register(moving, fixed, normals, dist_mode=mode, max_iterations=0)["stop"] == P.STOP_MAX_ITERATIONS
    # the solve on the smallest well-posed system: the identity asks for x = -g
    x, pivot = P.solve6(np.eye(6), np.arange(6.0))
    assert np.array_equal(x, -np.arange(6.0)) and pivot == 1.0
