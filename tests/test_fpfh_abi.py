"""CPU suite: the FPFH entry points exist, the ABI version is unchanged, and a null context is refused without a device and with the
outputs untouched."""
import ctypes as C

import numpy as np

import fpfh_reference as F

NAMES = ("mi_fpfh_features", "mi_fpfh_features_times")


def test_library_exports_the_fpfh_entry_points(capi):
    lib = capi.lib()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in capi.EXPORTS, name
    assert lib.mi_abi_version() == 4          # additive: no signature of version 4 changed
    assert (capi.FPFH_BINS, capi.FPFH_DIM) == (11, 33) == (F.BINS, F.DIM)
    for name in ("fpfh_features", "fpfh_features_times"):
        assert hasattr(capi.Context, name) and hasattr(capi, name + "_raw"), name


def test_the_header_declares_them(capi):
    import os
    from conftest import ROOT
    text = open(os.path.join(ROOT, "include", "mi_slam.h")).read()
    for name in NAMES:
        assert "int %s(mi_ctx* ctx" % name in text, name
    assert "#define MI_FPFH_BINS 11" in text and "#define MI_FPFH_DIM  33" in text and "#define MI_FPFH_STAGES 8" in text


def test_a_null_context_is_refused_without_a_device(capi):
    cloud, normals = np.zeros((4, 3), np.float32), np.tile(np.array([0, 0, 1], np.float32), (4, 1))
    fpfh, counts, count = np.full((4, 33), -7.5, np.float32), np.full((4, 33), 7, np.uint8), np.full(4, -7, np.int32)
    rc = capi.fpfh_features_raw(None, cloud.ctypes.data, normals.ctypes.data, 4, 3, 0, float("inf"), fpfh.ctypes.data, counts.ctypes.data, count.ctypes.data)
    assert rc == capi.MI_ERR_INVALID_ARG and capi.lib().mi_last_error().decode() == "mi_fpfh_features: null context"
    assert (fpfh == -7.5).all() and (counts == 7).all() and (count == -7).all()
    ms = (C.c_double * 8)(*([-7.5] * 8))
    assert capi.fpfh_features_times_raw(None, ms) == capi.MI_ERR_INVALID_ARG and list(ms) == [-7.5] * 8
    assert capi.lib().mi_last_error().decode().startswith("mi_fpfh_features_times")
