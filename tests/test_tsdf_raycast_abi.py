"""CPU suite: mi_tsdf_raycast exists -- the header declares it, its params struct and its limit, the library exports it, the binding types it
from the header -- the interface version has not moved, the struct is 64 bytes with the offsets the compiler gives it, the default params
hold the documented values, and a null context is refused without a device and with every output untouched."""
import ctypes as C
import os
import re

import numpy as np

from conftest import ROOT
from test_capi_prototypes import _compile

V, I, L = C.c_void_p, C.c_int, C.c_longlong


def test_the_header_declares_the_raycast_interface():
    text = open(os.path.join(ROOT, "include", "mi_slam.h")).read()
    for name in ("mi_tsdf_raycast_params_default", "mi_tsdf_raycast"):
        assert re.search(r"\b%s\s*\(" % name, text), name
    assert re.search(r"typedef struct mi_tsdf_raycast_params \{.*?\} mi_tsdf_raycast_params;", text, re.S)
    assert "#define MI_TSDF_RAYCAST_MAX_STEPS 65536" in text and "tests/tsdf_raycast_reference.py" in text


def test_library_exports_the_raycast_entry_points(capi):
    lib = capi.lib()
    protos = {p[0]: p for p in capi._PROTOTYPES}
    for name, restype, argtypes in (("mi_tsdf_raycast_params_default", None, [V]), ("mi_tsdf_raycast", I, [V, V, V, V, I, V, V, V, V, I, V, V, V, V])):
        assert hasattr(lib, name) and name in capi.EXPORTS, name
        f = getattr(lib, name)
        assert protos[name][3] is restype and protos[name][4] == argtypes, (name, protos[name][2])      # read from the header ...
        assert f.restype is restype and list(f.argtypes) == argtypes, name                               # ... and typed at load
    assert lib.mi_abi_version() == 4          # additive: no signature of version 4 changed
    assert callable(capi.Context.tsdf_raycast) and callable(capi.tsdf_raycast_params) and callable(capi.tsdf_raycast_raw)
    ray = open(os.path.join(ROOT, "cuda-slam_amd", "csrc", "tsdf_cast.hpp")).read()
    m = re.search(r"constexpr int TSDF_RAYCAST_MAX_STEPS = (\d+);", ray)
    assert m and int(m.group(1)) == capi.TSDF_RAYCAST_MAX_STEPS == 65536


def test_the_default_params_hold_the_documented_values(capi):
    p = capi.tsdf_raycast_params()
    assert [name for name, _ in capi.TsdfRaycast.Params._fields_] == ["voxel_size", "min_weight", "min_range", "max_range", "visit_every_sample", "reserved"]
    assert (p.voxel_size, p.min_weight, p.min_range, p.max_range, p.visit_every_sample) == (0.0, 1.0, 0.0, 0.0, 0) and list(p.reserved) == [0] * 11
    assert C.sizeof(capi.TsdfRaycast.Params) == 64
    q = capi.tsdf_raycast_params(voxel_size=0.1, max_range=4, visit_every_sample=1)
    assert (q.voxel_size, q.max_range, q.visit_every_sample) == (np.float32(0.1), 4.0, 1)
    capi.lib().mi_tsdf_raycast_params_default(None)          # a null pointer is ignored


def test_the_compiler_agrees_with_the_params_layout(capi, tmp_path):
    cls, ctype = capi.TsdfRaycast.Params, capi.TsdfRaycast.C_TYPE
    out = ['#include <cstddef>', '#include "mi_slam.h"', 'static_assert(sizeof(%s) == 64 && sizeof(%s) == %d, "%s: size");' % (ctype, ctype, C.sizeof(cls), ctype)]
    for field, ftype in cls._fields_:
        out.append('static_assert(offsetof(%s, %s) == %d, "%s.%s: offset");' % (ctype, field, getattr(cls, field).offset, ctype, field))
        out.append('static_assert(sizeof(%s::%s) == %d, "%s.%s: size");' % (ctype, field, C.sizeof(ftype), ctype, field))
    out.append("int main() { return 0; }")
    _compile(tmp_path, "tsdf_raycast_layout", "\n".join(out) + "\n")


def test_the_direction_helpers(capi):
    d = capi.pinhole_directions(4, 3, 2.0, 4.0, 1.5, 1.0)
    assert d.shape == (12, 3) and d.dtype == np.float32 and (d[:, 2] == 1).all()
    assert np.array_equal(d[0], [-0.75, -0.25, 1]) and np.array_equal(d[5], [-0.25, 0, 1]) and np.array_equal(d[11], [0.75, 0.25, 1])      # row v * width + u
    s = capi.spherical_directions(3, 8, -0.5, 0.5)
    assert s.shape == (24, 3) and np.abs(np.linalg.norm(s.astype(np.float64), axis=1) - 1).max() <= 1e-7
    assert np.allclose(s[0], [np.cos(0.5), 0, -np.sin(0.5)]) and np.allclose(s[8 + 2], [0, 1, 0], atol=1e-7) and np.allclose(s[16], [np.cos(0.5), 0, np.sin(0.5)])
    assert capi.spherical_directions(1, 4, 0.25, 9.0).shape == (4, 3)


def test_a_null_context_is_refused_without_a_device(capi):
    params = capi.tsdf_raycast_params(voxel_size=0.5, max_range=4.0)
    origin, dirs = np.zeros(3, np.float32), np.ones((2, 3), np.float32)
    depth, xyz, nrm, hits = np.full(2, -7.5, np.float32), np.full((2, 3), -7.5, np.float32), np.full((2, 3), -7.5, np.float32), C.c_longlong(-7)
    rc = capi.tsdf_raycast_raw(None, None, None, None, 0, origin.ctypes.data, C.addressof(params), None, dirs.ctypes.data, 2, depth.ctypes.data,
                               xyz.ctypes.data, nrm.ctypes.data, C.addressof(hits))
    msg = capi.lib().mi_last_error().decode()
    assert rc == capi.MI_ERR_INVALID_ARG and msg.startswith("mi_tsdf_raycast: null context"), (rc, msg)
    assert hits.value == -7 and (depth == -7.5).all() and (xyz == -7.5).all() and (nrm == -7.5).all()
