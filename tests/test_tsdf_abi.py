"""CPU suite: the TSDF entry points exist -- the header declares them, the params struct, its limit and MI_TSDF_STAGES, the library exports
them, the binding types them from the header -- the interface version has not moved, the default params hold the documented values, the
binding's constants are the kernels', and a null context is refused without a device and with every output untouched."""
import ctypes as C
import os
import re

import numpy as np

from conftest import ROOT
from test_capi_prototypes import _compile

NAMES = ("mi_tsdf_params_default", "mi_tsdf_integrate", "mi_tsdf_extract", "mi_tsdf_times")
V, I, F, L = C.c_void_p, C.c_int, C.c_float, C.c_longlong


def test_the_header_declares_the_tsdf_interface():
    text = open(os.path.join(ROOT, "include", "mi_slam.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, text), name
    assert re.search(r"typedef struct mi_tsdf_params \{.*?\} mi_tsdf_params;", text, re.S)
    for line in ("#define MI_TSDF_STAGES 8", "#define MI_TSDF_MAX_HALF_STEPS 16"):
        assert line in text, line
    assert "tests/tsdf_reference.py" in text


def test_library_exports_the_tsdf_entry_points(capi):
    lib = capi.lib()
    protos = {p[0]: p for p in capi._PROTOTYPES}
    for name, restype, argtypes in (("mi_tsdf_params_default", None, [V]),
                                    ("mi_tsdf_integrate", I, [V, V, V, I, V, V, V, V, V, V, I, V, V, V, L, V]),
                                    ("mi_tsdf_extract", I, [V, V, V, V, I, V, F, F, V, V, L, V]), ("mi_tsdf_times", I, [V, V])):
        assert hasattr(lib, name) and name in capi.EXPORTS, name
        f = getattr(lib, name)
        assert protos[name][3] is restype and protos[name][4] == argtypes, (name, protos[name][2])      # read from the header ...
        assert f.restype is restype and list(f.argtypes) == argtypes, name                               # ... and typed at load
    assert lib.mi_abi_version() == 4          # additive: no signature of version 4 changed
    assert len(capi.Context._TIMES["tsdf"]) == 8
    for method in ("tsdf_integrate", "tsdf_extract", "tsdf_times"):
        assert callable(getattr(capi.Context, method)), method
    assert callable(capi.tsdf_params) and callable(capi.tsdf_integrate_raw) and callable(capi.tsdf_extract_raw)


def test_the_default_params_hold_the_documented_values(capi):
    p = capi.tsdf_params()
    assert [name for name, _ in capi.Tsdf.Params._fields_] == ["voxel_size", "truncation", "min_range", "max_range", "max_weight", "reserved"]
    assert (p.voxel_size, p.truncation, p.min_range, p.max_range, p.max_weight) == (0.0, 0.0, 0.0, np.inf, np.inf) and list(p.reserved) == [0] * 11
    assert C.sizeof(capi.Tsdf.Params) == 64
    q = capi.tsdf_params(voxel_size=0.1, truncation=0.3, max_weight=8)
    assert (q.voxel_size, q.truncation, q.max_weight) == (np.float32(0.1), np.float32(0.3), 8.0)
    capi.lib().mi_tsdf_params_default(None)          # a null pointer is ignored


def test_the_compiler_agrees_with_the_params_layout(capi, tmp_path):
    cls, ctype = capi.Tsdf.Params, capi.Tsdf.C_TYPE
    out = ['#include <cstddef>', '#include "mi_slam.h"', 'static_assert(sizeof(%s) == %d, "%s: size");' % (ctype, C.sizeof(cls), ctype)]
    for field, ftype in cls._fields_:
        out.append('static_assert(offsetof(%s, %s) == %d, "%s.%s: offset");' % (ctype, field, getattr(cls, field).offset, ctype, field))
        out.append('static_assert(sizeof(%s::%s) == %d, "%s.%s: size");' % (ctype, field, C.sizeof(ftype), ctype, field))
    out.append("int main() { return 0; }")
    _compile(tmp_path, "tsdf_layout", "\n".join(out) + "\n")


def test_the_bindings_constants_are_the_kernels_and_the_headers(capi):
    text = open(os.path.join(ROOT, "cuda-slam_amd", "csrc", "kernels.h")).read()
    m = re.search(r"constexpr int TSDF_BLOCK = (\d+);", text)
    assert m and int(m.group(1)) == capi.TSDF_BLOCK
    ray = open(os.path.join(ROOT, "cuda-slam_amd", "csrc", "tsdf_ray.hpp")).read()
    m = re.search(r"constexpr int TSDF_MAX_HALF_STEPS = (\d+);", ray)
    assert m and int(m.group(1)) == capi.TSDF_MAX_HALF_STEPS == 16


def test_a_null_context_is_refused_without_a_device(capi):
    params = capi.tsdf_params(voxel_size=0.5, truncation=1.0)
    xyz, offsets, origin = np.ones((4, 3), np.float32), np.array([0, 4], np.int64), np.zeros(3, np.float32)
    coord, tsdf, weight = np.full((8, 3), -7, np.int32), np.full(8, -7.5, np.float32), np.full(8, -7.5, np.float32)
    nv = C.c_longlong(-7)
    rc = capi.tsdf_integrate_raw(None, xyz.ctypes.data, offsets.ctypes.data, 1, None, origin.ctypes.data, C.addressof(params), None, None, None, 0,
                                 coord.ctypes.data, tsdf.ctypes.data, weight.ctypes.data, 8, C.addressof(nv))
    msg = capi.lib().mi_last_error().decode()
    assert rc == capi.MI_ERR_INVALID_ARG and msg.startswith("mi_tsdf_integrate: null context"), (rc, msg)
    assert nv.value == -7 and (coord == -7).all() and (tsdf == -7.5).all() and (weight == -7.5).all()
    one = (np.zeros((1, 3), np.int32), np.zeros(1, np.float32), np.ones(1, np.float32))
    out_xyz, out_n = np.full((3, 3), -7.5, np.float32), np.full((3, 3), -7.5, np.float32)
    rc = capi.tsdf_extract_raw(None, one[0].ctypes.data, one[1].ctypes.data, one[2].ctypes.data, 1, origin.ctypes.data, 0.5, 1.0, out_xyz.ctypes.data,
                               out_n.ctypes.data, 3, C.addressof(nv))
    msg = capi.lib().mi_last_error().decode()
    assert rc == capi.MI_ERR_INVALID_ARG and msg.startswith("mi_tsdf_extract: null context"), (rc, msg)
    assert nv.value == -7 and (out_xyz == -7.5).all() and (out_n == -7.5).all()
    out = (C.c_double * 8)(*([-7.0] * 8))
    assert capi.lib().mi_tsdf_times(None, out) == capi.MI_ERR_INVALID_ARG and list(out) == [-7.0] * 8
    assert capi.lib().mi_last_error().decode().startswith("mi_tsdf_times")
