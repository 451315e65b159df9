"""CPU suite: the generalized-ICP entry points exist, the ABI version is unchanged, and a null context is refused without a device and with
the outputs untouched."""
import ctypes as C

import numpy as np

import gicp_reference as G

NAMES = ("mi_estimate_covariances", "mi_icp_gicp_register", "mi_gicp_system", "mi_icp_gicp_times")


def test_library_exports_the_gicp_entry_points(capi):
    lib = capi.lib()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in capi.EXPORTS, name
    assert lib.mi_abi_version() == 4          # additive: no signature of version 4 changed
    assert (capi.COV_RAW, capi.COV_PLANE) == (0, 1) == (G.COV_RAW, G.COV_PLANE)
    for name in ("estimate_covariances", "icp_gicp_register", "gicp_system", "icp_gicp_times"):
        assert hasattr(capi.Context, name) and hasattr(capi, name + "_raw"), name


def test_the_header_declares_them(capi):
    import os
    from conftest import ROOT
    text = open(os.path.join(ROOT, "include", "mi_slam.h")).read()
    for name in NAMES:
        assert "int %s(mi_ctx* ctx" % name in text, name
    assert "#define MI_COV_RAW   0" in text and "#define MI_COV_PLANE 1" in text and "#define MI_GICP_STAGES 8" in text


def test_a_null_context_is_refused_without_a_device(capi):
    cloud, cov = np.zeros((4, 3), np.float32), np.tile(np.array([1, 0, 0, 1, 0, 1], np.float32), (4, 1))
    T, it, err, why = np.full(16, -7.5, np.float32), C.c_int(-7), C.c_float(-7.5), C.c_int(-7)
    p = capi.plane_params()
    rc = capi.icp_gicp_register_raw(None, cloud.ctypes.data, cov.ctypes.data, 4, cloud.ctypes.data, cov.ctypes.data, 4, C.addressof(p), None, T.ctypes.data,
                                    C.addressof(it), C.addressof(err), C.addressof(why))
    assert rc == capi.MI_ERR_INVALID_ARG and capi.lib().mi_last_error().decode() == "mi_icp_gicp_register: null context"
    assert (T == -7.5).all() and it.value == -7 and err.value == -7.5 and why.value == -7
    sums, centre, idx = np.full(32, -7.5), np.full(3, -7.5, np.float32), np.full(4, -7, np.int32)
    rc = capi.gicp_system_raw(None, cloud.ctypes.data, cov.ctypes.data, 4, cloud.ctypes.data, cov.ctypes.data, 4, None, capi.DIST_FMA, float("inf"),
                              sums.ctypes.data, centre.ctypes.data, idx.ctypes.data)
    assert rc == capi.MI_ERR_INVALID_ARG and capi.lib().mi_last_error().decode() == "mi_gicp_system: null context"
    assert (sums == -7.5).all() and (centre == -7.5).all() and (idx == -7).all()
    out, count = np.full((4, 6), -7.5, np.float32), np.full(4, -7, np.int32)
    rc = capi.estimate_covariances_raw(None, cloud.ctypes.data, 4, 3, 0, float("inf"), capi.COV_PLANE, 1e-3, out.ctypes.data, count.ctypes.data)
    assert rc == capi.MI_ERR_INVALID_ARG and capi.lib().mi_last_error().decode() == "mi_estimate_covariances: null context"
    assert (out == -7.5).all() and (count == -7).all()
    ms = (C.c_double * 8)(*([-7.5] * 8))
    assert capi.icp_gicp_times_raw(None, ms) == capi.MI_ERR_INVALID_ARG and list(ms) == [-7.5] * 8
    assert capi.lib().mi_last_error().decode().startswith("mi_icp_gicp_times")
