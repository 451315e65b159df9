"""CPU suite: mi_evaluate_registration and its *_times exist, the interface version has not moved, and a null context is refused without a
device and with every output untouched."""
import ctypes as C

import numpy as np


def test_library_exports_the_evaluation_entry_points(capi):
    lib = capi.lib()
    V, I, F = C.c_void_p, C.c_int, C.c_float
    for name, argtypes in (("mi_evaluate_registration", [V, V, I, V, I, V, V, I, F, V, V, V, V, V, V]), ("mi_evaluate_registration_times", [V, V])):
        assert hasattr(lib, name), name
        assert name in capi.EXPORTS, name
        f = getattr(lib, name)
        assert f.restype is C.c_int and list(f.argtypes) == argtypes, name
    assert lib.mi_abi_version() == 4          # additive: no signature of version 4 changed
    assert len(capi.Context._TIMES["evaluate_registration"]) == 8


def test_a_null_context_is_refused_without_a_device(capi):
    cloud = np.zeros((4, 3), np.float32)
    pairs = np.arange(4, dtype=np.int32)
    for given in (None, pairs.ctypes.data):
        fitness, rmse = C.c_double(-7.5), C.c_double(-7.5)
        sums, info, idx, d2 = np.full(32, -7.5), np.full(36, -7.5), np.full(4, -7, np.int32), np.full(4, -7.5, np.float32)
        rc = capi.evaluate_registration_raw(None, cloud.ctypes.data, 4, cloud.ctypes.data, 4, None, given, capi.DIST_FMA, float("inf"), C.addressof(fitness),
                                            C.addressof(rmse), sums.ctypes.data, info.ctypes.data, idx.ctypes.data, d2.ctypes.data)
        msg = capi.lib().mi_last_error().decode()
        assert rc == capi.MI_ERR_INVALID_ARG and msg.startswith("mi_evaluate_registration: null context"), (rc, msg)
        assert fitness.value == -7.5 and rmse.value == -7.5
        assert (sums == -7.5).all() and (info == -7.5).all() and (idx == -7).all() and (d2 == -7.5).all()


def test_the_times_call_refuses_null(capi):
    out = (C.c_double * 8)(*([-7.0] * 8))
    assert capi.lib().mi_evaluate_registration_times(None, out) == capi.MI_ERR_INVALID_ARG and list(out) == [-7.0] * 8
    assert capi.lib().mi_last_error().decode().startswith("mi_evaluate_registration_times")
