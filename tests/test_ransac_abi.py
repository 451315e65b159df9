"""CPU suite: the hypothesise-and-verify entry points exist, the ABI version is unchanged, and a null context is refused without a device
and with the outputs untouched."""
import ctypes as C

import numpy as np

NAMES = ("mi_ransac_register", "mi_ransac_hypotheses", "mi_ransac_register_times")


def test_library_exports_the_ransac_entry_points(capi):
    lib = capi.lib()
    for name in NAMES + ("mi_ransac_params_default",):
        assert hasattr(lib, name), name
        assert name in capi.EXPORTS, name
    assert lib.mi_abi_version() == 4          # additive: no signature of version 4 changed
    for name in ("ransac_register", "ransac_hypotheses", "ransac_register_times"):
        assert hasattr(capi.Context, name) and hasattr(capi, name + "_raw"), name
    p = capi.ransac_params(0.05)
    assert (p.hypotheses, p.seed, p.refine_iterations, list(p.reserved)) == (100000, 0, 2, [0] * 8)
    assert abs(p.edge_similarity - 0.9) < 1e-7 and abs(p.max_distance - 0.05) < 1e-9
    assert C.sizeof(capi.RansacParams) == 64  # int, pad, u64, 2 floats, int, 8 ints, pad


def test_the_header_declares_them(capi):
    import os
    from conftest import ROOT
    text = open(os.path.join(ROOT, "include", "mi_slam.h")).read()
    for name in NAMES:
        assert "int %s(mi_ctx* ctx" % name in text, name
    assert "void mi_ransac_params_default(mi_ransac_params* params);" in text and "#define MI_RANSAC_STAGES 8" in text
    assert "0xBF58476D1CE4E5B9" in text and "0x94D049BB133111EB" in text and "0x9E3779B97F4A7C15" in text


def test_a_null_context_is_refused_without_a_device(capi):
    src = np.zeros((4, 3), np.float32)
    idx = np.arange(4, dtype=np.int32)
    p = capi.ransac_params(0.1)
    R9, t3, mask = np.full(9, -7.5, np.float32), np.full(3, -7.5, np.float32), np.full(4, 7, np.uint8)
    scal = np.full(4, -7, np.int32)
    rmse = np.full(1, -7.5, np.float32)
    rc = capi.ransac_register_raw(None, src.ctypes.data, 4, src.ctypes.data, 4, idx.ctypes.data, C.addressof(p), R9.ctypes.data, t3.ctypes.data,
                                  scal[0:].ctypes.data, rmse.ctypes.data, scal[1:].ctypes.data, scal[2:].ctypes.data, mask.ctypes.data)
    assert rc == capi.MI_ERR_INVALID_ARG and capi.lib().mi_last_error().decode() == "mi_ransac_register: null context"
    assert (R9 == -7.5).all() and (t3 == -7.5).all() and (scal == -7).all() and (mask == 7).all() and rmse[0] == -7.5
    tri = np.full(6, -7, np.int32)
    rc = capi.ransac_hypotheses_raw(None, src.ctypes.data, 4, src.ctypes.data, 4, idx.ctypes.data, C.addressof(p), 0, 2, tri.ctypes.data, None, None, None)
    assert rc == capi.MI_ERR_INVALID_ARG and capi.lib().mi_last_error().decode() == "mi_ransac_hypotheses: null context" and (tri == -7).all()
    ms = (C.c_double * 8)(*([-7.5] * 8))
    assert capi.ransac_register_times_raw(None, ms) == capi.MI_ERR_INVALID_ARG and list(ms) == [-7.5] * 8
    assert capi.lib().mi_last_error().decode().startswith("mi_ransac_register_times")
