"""CPU suite: the descriptor-matching entry points exist, the ABI version is unchanged, and a null context is refused without a device
and with the outputs untouched."""
import ctypes as C

import numpy as np

import match_reference as M

NAMES = ("mi_feature_match", "mi_feature_match_times")


def test_library_exports_the_matching_entry_points(capi):
    lib = capi.lib()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in capi.EXPORTS, name
    assert lib.mi_abi_version() == 4          # additive: no signature of version 4 changed
    assert capi.FEATURE_MAX_DIM == 64 == M.MAX_DIM
    for name in ("feature_match", "feature_match_times"):
        assert hasattr(capi.Context, name) and hasattr(capi, name + "_raw"), name


def test_the_header_declares_them(capi):
    import os
    from conftest import ROOT
    text = open(os.path.join(ROOT, "include", "mi_slam.h")).read()
    for name in NAMES:
        assert "int %s(mi_ctx* ctx" % name in text, name
    assert "#define MI_FEATURE_MAX_DIM 64" in text and "#define MI_MATCH_STAGES 8" in text
    assert "Matching the descriptors is the caller's" not in text


def test_a_null_context_is_refused_without_a_device(capi):
    q, t = np.ones((4, 33), np.float32), np.ones((5, 33), np.float32)
    idx, d2 = np.full(4, -7, np.int32), np.full(4, -7.5, np.float32)
    rc = capi.feature_match_raw(None, q.ctypes.data, 4, t.ctypes.data, 5, 33, 1, idx.ctypes.data, d2.ctypes.data)
    assert rc == capi.MI_ERR_INVALID_ARG and capi.lib().mi_last_error().decode() == "mi_feature_match: null context"
    assert (idx == -7).all() and (d2 == -7.5).all()
    ms = (C.c_double * 8)(*([-7.5] * 8))
    assert capi.feature_match_times_raw(None, ms) == capi.MI_ERR_INVALID_ARG and list(ms) == [-7.5] * 8
    assert capi.lib().mi_last_error().decode().startswith("mi_feature_match_times")
