"""CPU suite: the radius-search entry points exist with the header's prototypes, typed at load, and the ABI is still version 4; the binding's
constants are the header's and the kernels'; the refusals that need no device (a NULL context; the ones that need a context:
tests/test_gpu_radius.py) leave every output untouched."""
import ctypes as C
import os
import re

import numpy as np

V, I, F, LL = C.c_void_p, C.c_int, C.c_float, C.c_longlong


def test_library_exports_the_radius_entry_points(capi):
    lib = capi.lib()
    protos = {p[0]: p for p in capi._PROTOTYPES}
    for name, argtypes in (("mi_radius_search", [V, V, I, V, I, F, I, I, V, V, V, LL, V]), ("mi_radius_search_times", [V, V]),
                           ("mi_selftest_radius_grid", [V, V])):
        assert hasattr(lib, name) and name in capi.EXPORTS, name
        assert protos[name][4] == argtypes and list(getattr(lib, name).argtypes) == argtypes, (name, protos[name][2])      # typed at load
        assert protos[name][3] is I
    assert lib.mi_abi_version() == 4          # additive: no signature of version 4 changed
    text = open(capi._HEADER).read()
    assert "#define MI_RADIUS_STAGES 8" in text and "#define MI_RADIUS_MAX_TOTAL (1LL << 31)" in text and capi.RADIUS_MAX_TOTAL == 1 << 31
    for name in ("radius_search", "radius_count", "radius_search_times", "radius_grid"):
        assert callable(getattr(capi.Context, name))
    assert callable(capi.radius_search_raw) and len(capi.Context._TIMES["radius_search"]) == 8


def test_the_bindings_sort_limits_are_read_from_the_kernels_header(capi):
    text = open(os.path.join(os.path.dirname(capi._HEADER), "..", "cuda-slam_amd", "csrc", "kernels.h")).read()
    for name in ("RADIUS_WAVE_ROW", "RADIUS_SORT_CHUNK"):
        m = re.search(r"constexpr int %s = (\d+);" % name, text)
        assert m and int(m.group(1)) == getattr(capi, name), name
    assert capi.RADIUS_WAVE_ROW == 64 and capi.RADIUS_SORT_CHUNK >= 2 * capi.RADIUS_WAVE_ROW
    assert capi.RADIUS_SORT_CHUNK & (capi.RADIUS_SORT_CHUNK - 1) == 0


def test_a_null_context_is_refused_without_a_device(capi):
    cloud = np.zeros((4, 3), np.float32)
    offsets, idx, d2 = np.full(5, -7, np.int64), np.full(16, -7, np.int32), np.full(16, -7.5, np.float32)
    total = C.c_longlong(-7)
    for queries in (None, cloud.ctypes.data):
        for lists in (True, False):
            rc = capi.radius_search_raw(None, queries, 4, cloud.ctypes.data, 4, 1.0, capi.DIST_CPU_ROUNDING, 1, offsets.ctypes.data,
                                        idx.ctypes.data if lists else None, d2.ctypes.data if lists else None, 16 if lists else 0, C.addressof(total))
            msg = capi.lib().mi_last_error().decode()
            assert rc == capi.MI_ERR_INVALID_ARG and msg.startswith("mi_radius_search") and "null context" in msg
            assert (offsets == -7).all() and (idx == -7).all() and (d2 == -7.5).all() and total.value == -7
    out = (C.c_double * 8)(*([-7.0] * 8))
    assert capi.lib().mi_radius_search_times(None, out) == capi.MI_ERR_INVALID_ARG and list(out) == [-7.0] * 8
    assert capi.lib().mi_last_error().decode().startswith("mi_radius_search_times")
    dims = (C.c_int * 3)(-7, -7, -7)
    assert capi.lib().mi_selftest_radius_grid(None, dims) == capi.MI_ERR_INVALID_ARG and list(dims) == [-7, -7, -7]
