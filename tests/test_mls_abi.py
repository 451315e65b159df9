"""CPU suite: the moving-least-squares entry points exist with the header's prototypes, typed at load; mi_mls_params is 64 bytes with the
header's layout and mi_mls_params_default gives the header's defaults; the refusals that need no device (a NULL context; the ones that
need a context: tests/test_gpu_mls.py) leave every output untouched."""
import ctypes as C

import numpy as np
import pytest

from test_capi_prototypes import _compile

V, I = C.c_void_p, C.c_int


def test_library_exports_the_mls_entry_points(capi):
    lib = capi.lib()
    protos = {p[0]: p for p in capi._PROTOTYPES}
    for name, argtypes in (("mi_mls_smooth", [V, V, I, V, I, V, V, V, V, V, V]), ("mi_mls_smooth_times", [V, V]), ("mi_mls_params_default", [V])):
        assert hasattr(lib, name) and name in capi.EXPORTS, name
        assert protos[name][4] == argtypes and list(getattr(lib, name).argtypes) == argtypes, (name, protos[name][2])      # typed at load
    assert protos["mi_mls_smooth"][3] is I and protos["mi_mls_params_default"][3] is None
    assert lib.mi_abi_version() == 4          # additive: no signature of version 4 changed
    text = open(capi._HEADER).read()
    assert "#define MI_MLS_STAGES 8" in text
    for name, value in (("QUADRATIC", 0), ("PLANE", 1), ("UNTOUCHED", 2)):
        assert "#define MI_MLS_%s %d" % (name, value) in text and getattr(capi.Mls, name) == value
    for name in ("mls_smooth", "mls_smooth_times"):
        assert callable(getattr(capi.Context, name))
    assert len(capi.Context._TIMES["mls_smooth"]) == 8


def test_the_compiler_agrees_with_the_params_layout(capi, tmp_path):
    cls, ctype = capi.Mls.Params, capi.Mls.C_TYPE
    assert C.sizeof(cls) == 64
    out = ['#include <cstddef>', '#include "mi_slam.h"', 'static_assert(sizeof(%s) == %d, "%s: size");' % (ctype, C.sizeof(cls), ctype)]
    for field, ftype in cls._fields_:
        out.append('static_assert(offsetof(%s, %s) == %d, "%s.%s: offset");' % (ctype, field, getattr(cls, field).offset, ctype, field))
        out.append('static_assert(sizeof(%s::%s) == %d, "%s.%s: size");' % (ctype, field, C.sizeof(ftype), ctype, field))
    out.append("int main() { return 0; }")
    _compile(tmp_path, "mls_layout", "\n".join(out) + "\n")


def test_defaults_are_the_documented_ones(capi):
    p = capi.Mls.Params()
    C.memset(C.addressof(p), 0xFF, C.sizeof(p))
    capi.lib().mi_mls_params_default(C.byref(p))
    assert (p.radius, p.gauss_scale) == (0.0, 0.0)                             # the caller must set the radius; 0: the radius is the scale
    assert (p.order, p.min_neighbours, p.dist_mode) == (2, 3, capi.DIST_CPU_ROUNDING) and list(p.reserved) == [0] * 11
    capi.lib().mi_mls_params_default(None)                                     # a NULL struct is ignored
    q = capi.mls_params(radius=0.9, gauss_scale=0.45, order=1, min_neighbours=7, dist_mode=capi.DIST_FMA)
    assert (q.radius, q.gauss_scale) == (float(np.float32(0.9)), float(np.float32(0.45)))
    assert (q.order, q.min_neighbours, q.dist_mode) == (1, 7, capi.DIST_FMA)
    with pytest.raises(TypeError):
        capi.mls_params(no_such_field=1)
    with pytest.raises(TypeError):
        capi.mls_params(reserved=1)


def test_a_null_context_is_refused_without_a_device(capi):
    cloud = np.zeros((4, 3), np.float32)
    xyz, normals, curvature = np.full((4, 3), -7.5, np.float32), np.full((4, 3), -7.5, np.float32), np.full(4, -7.5, np.float32)
    neighbours, status = np.full(4, -7, np.int32), np.full(4, 7, np.uint8)
    p = capi.mls_params(radius=1.0)
    for queries in (None, cloud.ctypes.data):
        rc = capi.mls_smooth_raw(None, cloud.ctypes.data, 4, queries, 4, C.addressof(p), xyz.ctypes.data, normals.ctypes.data, curvature.ctypes.data,
                                 neighbours.ctypes.data, status.ctypes.data)
        msg = capi.lib().mi_last_error().decode()
        assert rc == capi.MI_ERR_INVALID_ARG and msg.startswith("mi_mls_smooth") and "null context" in msg
        assert (xyz == -7.5).all() and (normals == -7.5).all() and (curvature == -7.5).all() and (neighbours == -7).all() and (status == 7).all()
    out = (C.c_double * 8)(*([-7.0] * 8))
    assert capi.lib().mi_mls_smooth_times(None, out) == capi.MI_ERR_INVALID_ARG and list(out) == [-7.0] * 8
    assert capi.lib().mi_last_error().decode().startswith("mi_mls_smooth_times")
