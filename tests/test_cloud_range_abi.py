"""CPU suite: mi_selftest_cloud_range exists and refuses bad arguments before it touches a device or the context."""
import ctypes as C

import numpy as np


def test_cloud_range_selftest_is_exported_and_refuses_bad_arguments(capi):
    lib = capi.lib()
    assert hasattr(lib, "mi_selftest_cloud_range") and "mi_selftest_cloud_range" in capi.EXPORTS
    assert lib.mi_abi_version() == 4          # additive: no signature of version 4 changed
    p = np.ones((4, 3), np.float32)
    lo_hi = np.full(6, -7.0, np.float32)
    bad = C.c_int(-7)
    fake_ctx = C.create_string_buffer(64)     # never looked into: every refusal below comes before the context is used
    f = capi.selftest_cloud_range_raw
    cases = {
        "null context": (None, p.ctypes.data, 4, 0, lo_hi.ctypes.data, C.byref(bad)),
        "null cloud": (C.addressof(fake_ctx), None, 4, 0, lo_hi.ctypes.data, C.byref(bad)),
        "null lo_hi": (C.addressof(fake_ctx), p.ctypes.data, 4, 0, None, C.byref(bad)),
        "null index": (C.addressof(fake_ctx), p.ctypes.data, 4, 0, lo_hi.ctypes.data, None),
        "n = 0": (C.addressof(fake_ctx), p.ctypes.data, 0, 0, lo_hi.ctypes.data, C.byref(bad)),
        "n < 0": (C.addressof(fake_ctx), p.ctypes.data, -1, 0, lo_hi.ctypes.data, C.byref(bad)),
        "check = -1": (C.addressof(fake_ctx), p.ctypes.data, 4, -1, lo_hi.ctypes.data, C.byref(bad)),
        "check = 3": (C.addressof(fake_ctx), p.ctypes.data, 4, 3, lo_hi.ctypes.data, C.byref(bad)),
    }
    for name, args in cases.items():
        assert f(*args) == capi.MI_ERR_INVALID_ARG, name
        assert "mi_selftest_cloud_range" in lib.mi_last_error().decode(), name
    assert (lo_hi == -7.0).all() and bad.value == -7
