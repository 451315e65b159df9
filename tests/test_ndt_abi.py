"""CPU suite: the NDT entry points exist, the ABI version is unchanged, a null context is refused without a device and with the outputs
untouched, and mi_ndt_constants -- a pure host function -- agrees with numpy's evaluation of the same formulas."""
import ctypes as C

import numpy as np

import ndt_reference as N

NAMES = ("mi_ndt_constants", "mi_ndt_voxels", "mi_ndt_params_default", "mi_ndt_register", "mi_ndt_system", "mi_ndt_times")


def test_library_exports_the_ndt_entry_points(capi):
    lib = capi.lib()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in capi.EXPORTS, name
    assert lib.mi_abi_version() == 4          # additive: no signature of version 4 changed
    for name in ("ndt_voxels", "ndt_register", "ndt_system", "ndt_times"):
        assert hasattr(capi.Context, name) and hasattr(capi, name + "_raw"), name
    p = capi.ndt_params()
    assert (p.eps_rotation, p.eps_translation, p.max_iterations, p.neighbourhood, p.sync_every, p.verbose) == (np.float32(1e-6), np.float32(1e-6), 50, 7, 0, 0)
    assert p.outlier_ratio == np.float32(0.55) and list(p.reserved) == [0] * 9 and C.sizeof(p) == 64


def test_the_header_declares_them(capi):
    import os
    from conftest import ROOT
    text = open(os.path.join(ROOT, "include", "mi_slam.h")).read()
    for name in ("mi_ndt_voxels", "mi_ndt_register", "mi_ndt_system", "mi_ndt_times"):
        assert "int %s(mi_ctx* ctx" % name in text, name
    assert "int mi_ndt_constants(float voxel_size, float outlier_ratio, double out[4]);" in text
    assert "void mi_ndt_params_default(mi_ndt_params* p);" in text and "#define MI_NDT_STAGES 8" in text


def test_a_null_context_is_refused_without_a_device(capi):
    cloud = np.zeros((4, 3), np.float32)
    coord, mean, icov = np.zeros((1, 3), np.int32), np.zeros((1, 3), np.float32), np.array([[1, 0, 0, 1, 0, 1]], np.float32)
    origin = np.zeros(3, np.float32)
    T, it, score, why = np.full(16, -7.5, np.float32), C.c_int(-7), C.c_float(-7.5), C.c_int(-7)
    p = capi.ndt_params()
    rc = capi.ndt_register_raw(None, cloud.ctypes.data, 4, coord.ctypes.data, mean.ctypes.data, icov.ctypes.data, 1, 1.0, origin.ctypes.data, C.addressof(p), None,
                               T.ctypes.data, C.addressof(it), C.addressof(score), C.addressof(why))
    assert rc == capi.MI_ERR_INVALID_ARG and capi.lib().mi_last_error().decode() == "mi_ndt_register: null context"
    assert (T == -7.5).all() and it.value == -7 and score.value == -7.5 and why.value == -7
    sums, centre, idx, terms = np.full(32, -7.5), np.full(3, -7.5, np.float32), np.full(4, -7, np.int32), np.full(4, 77, np.uint8)
    rc = capi.ndt_system_raw(None, cloud.ctypes.data, 4, coord.ctypes.data, mean.ctypes.data, icov.ctypes.data, 1, 1.0, origin.ctypes.data, None, 7, 0.55,
                             sums.ctypes.data, centre.ctypes.data, idx.ctypes.data, terms.ctypes.data)
    assert rc == capi.MI_ERR_INVALID_ARG and capi.lib().mi_last_error().decode() == "mi_ndt_system: null context"
    assert (sums == -7.5).all() and (centre == -7.5).all() and (idx == -7).all() and (terms == 77).all()
    oc, om, oi = np.full((4, 3), -7, np.int32), np.full((4, 3), -7.5, np.float32), np.full((4, 6), -7.5, np.float32)
    on, ocount, ocov, oo = C.c_int(-7), np.full(4, -7, np.int32), np.full((4, 6), -7.5, np.float32), np.full(3, -7.5, np.float32)
    rc = capi.ndt_voxels_raw(None, cloud.ctypes.data, 4, 1.0, None, 6, 0.01, oc.ctypes.data, om.ctypes.data, oi.ctypes.data, C.addressof(on), ocount.ctypes.data,
                             ocov.ctypes.data, oo.ctypes.data)
    assert rc == capi.MI_ERR_INVALID_ARG and capi.lib().mi_last_error().decode() == "mi_ndt_voxels: null context"
    assert (oc == -7).all() and (om == -7.5).all() and (oi == -7.5).all() and on.value == -7 and (ocount == -7).all() and (ocov == -7.5).all() and (oo == -7.5).all()
    ms = (C.c_double * 8)(*([-7.5] * 8))
    assert capi.ndt_times_raw(None, ms) == capi.MI_ERR_INVALID_ARG and list(ms) == [-7.5] * 8
    assert capi.lib().mi_last_error().decode().startswith("mi_ndt_times")


def test_the_constants_against_numpy(capi):
    for voxel, ratio in ((0.5, 0.55), (1.0, 0.55), (2.0, 0.3)):
        got, want = capi.ndt_constants(voxel, ratio), N.constants(voxel, ratio)
        ulps = np.abs(got - want) / np.spacing(np.abs(want))
        print("constants(%g, %g) = %s: %s units of the last place from numpy's" % (voxel, ratio, got, ulps))
        assert (ulps <= 4).all()
        assert got[0] < 0 < got[1] and got[2] == -0.5 * got[1] and got[3] == -(got[0] * got[1])
    out = np.full(4, -7.5)
    for voxel, ratio in ((0.0, 0.55), (-1.0, 0.55), (float("nan"), 0.55), (float("inf"), 0.55), (1.0, 0.0), (1.0, 1.0), (1.0, -0.1), (1.0, float("nan"))):
        assert capi.ndt_constants_raw(voxel, ratio, out.ctypes.data) == capi.MI_ERR_INVALID_ARG, (voxel, ratio)
        assert capi.lib().mi_last_error().decode().startswith("mi_ndt_constants") and (out == -7.5).all()
    assert capi.ndt_constants_raw(1.0, 0.55, None) == capi.MI_ERR_INVALID_ARG
