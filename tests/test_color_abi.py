"""CPU suite: the colored-ICP entry points exist, the ABI version is unchanged, and a null context is refused without a device and with the
outputs untouched."""
import ctypes as C

import numpy as np

import color_reference as CR

NAMES = ("mi_estimate_color_gradients", "mi_icp_color_register", "mi_color_system", "mi_icp_color_times")


def test_library_exports_the_color_entry_points(capi):
    lib = capi.lib()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in capi.EXPORTS, name
    assert [n for n in capi.EXPORTS if n in NAMES] == list(NAMES)          # in the header's order
    assert lib.mi_abi_version() == 4          # additive: no signature of version 4 changed
    for name in ("estimate_color_gradients", "icp_color_register", "color_system", "icp_color_times"):
        assert hasattr(capi.Context, name) and hasattr(capi, name + "_raw"), name


def test_the_header_declares_them(capi):
    import os
    from conftest import ROOT
    text = open(os.path.join(ROOT, "include", "mi_slam.h")).read()
    for name in NAMES:
        assert "int %s(mi_ctx* ctx" % name in text, name
    assert "#define MI_COLOR_STAGES 8" in text


def test_intensity_of_rgb_is_the_float32_mean_in_the_stated_order(capi):
    rng = np.random.default_rng(2)
    rgb = rng.uniform(0, 1, (500, 3)).astype(np.float32)
    got = capi.intensity_of_rgb(rgb)
    want = ((rgb[:, 0] + rgb[:, 1]) + rgb[:, 2]) / np.float32(3)
    assert got.dtype == np.float32 and got.shape == (500,) and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(got.view(np.uint32), CR.intensity_of_rgb(rgb).view(np.uint32))
    assert np.array_equal(capi.intensity_of_rgb(rgb.astype(np.float64).tolist()), got)


def test_a_null_context_is_refused_without_a_device(capi):
    cloud, up, I = np.zeros((4, 3), np.float32), np.tile(np.array([0, 0, 1], np.float32), (4, 1)), np.zeros(4, np.float32)
    T, it, err, why = np.full(16, -7.5, np.float32), C.c_int(-7), C.c_float(-7.5), C.c_int(-7)
    p = capi.plane_params()
    rc = capi.icp_color_register_raw(None, cloud.ctypes.data, I.ctypes.data, 4, cloud.ctypes.data, up.ctypes.data, I.ctypes.data, cloud.ctypes.data, 4,
                                     C.addressof(p), 0.968, None, T.ctypes.data, C.addressof(it), C.addressof(err), C.addressof(why))
    assert rc == capi.MI_ERR_INVALID_ARG and capi.lib().mi_last_error().decode() == "mi_icp_color_register: null context"
    assert (T == -7.5).all() and it.value == -7 and err.value == -7.5 and why.value == -7
    sums, centre, idx = np.full(32, -7.5), np.full(3, -7.5, np.float32), np.full(4, -7, np.int32)
    rc = capi.color_system_raw(None, cloud.ctypes.data, I.ctypes.data, 4, cloud.ctypes.data, up.ctypes.data, I.ctypes.data, cloud.ctypes.data, 4, None,
                               capi.DIST_FMA, float("inf"), 0.968, sums.ctypes.data, centre.ctypes.data, idx.ctypes.data)
    assert rc == capi.MI_ERR_INVALID_ARG and capi.lib().mi_last_error().decode() == "mi_color_system: null context"
    assert (sums == -7.5).all() and (centre == -7.5).all() and (idx == -7).all()
    out, count = np.full((4, 3), -7.5, np.float32), np.full(4, -7, np.int32)
    rc = capi.estimate_color_gradients_raw(None, cloud.ctypes.data, up.ctypes.data, I.ctypes.data, 4, 3, 0, float("inf"), out.ctypes.data, count.ctypes.data)
    assert rc == capi.MI_ERR_INVALID_ARG and capi.lib().mi_last_error().decode() == "mi_estimate_color_gradients: null context"
    assert (out == -7.5).all() and (count == -7).all()
    ms = (C.c_double * 8)(*([-7.5] * 8))
    assert capi.icp_color_times_raw(None, ms) == capi.MI_ERR_INVALID_ARG and list(ms) == [-7.5] * 8
    assert capi.lib().mi_last_error().decode().startswith("mi_icp_color_times")
