"""CPU suite: the place-recognition entry points exist -- the header declares them, the params struct, its limits and MI_SCAN_CONTEXT_STAGES,
the library exports them, the binding types them from the header -- the interface version has not moved, the default params hold the
documented values, the binding's constants are the kernels', the host-only tables call refuses what it must, and a null context is refused
without a device and with every output untouched."""
import ctypes as C
import os
import re

import numpy as np

from conftest import ROOT
from test_capi_prototypes import _compile

NAMES = ("mi_scan_context_params_default", "mi_scan_context_tables", "mi_scan_context", "mi_scan_context_search", "mi_scan_context_times")
V, I = C.c_void_p, C.c_int


def test_the_header_declares_the_scan_context_interface():
    text = open(os.path.join(ROOT, "include", "mi_slam.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, text), name
    assert re.search(r"typedef struct mi_scan_context_params \{.*?\} mi_scan_context_params;", text, re.S)
    for line in ("#define MI_SCAN_CONTEXT_STAGES 8", "#define MI_SCAN_CONTEXT_MAX_RINGS 32", "#define MI_SCAN_CONTEXT_MAX_SECTORS 64",
                 "#define MI_SCAN_CONTEXT_MAX_ROWS (1 << 26)"):
        assert line in text, line


def test_library_exports_the_scan_context_entry_points(capi):
    lib = capi.lib()
    protos = {p[0]: p for p in capi._PROTOTYPES}
    for name, restype, argtypes in (("mi_scan_context_params_default", None, [V]), ("mi_scan_context_tables", I, [V, V, V]),
                                    ("mi_scan_context", I, [V, V, V, I, V, V, V]),
                                    ("mi_scan_context_search", I, [V, V, I, V, I, V, V, V, V, V, V]), ("mi_scan_context_times", I, [V, V])):
        assert hasattr(lib, name) and name in capi.EXPORTS, name
        f = getattr(lib, name)
        assert protos[name][3] is restype and protos[name][4] == argtypes, (name, protos[name][2])      # read from the header ...
        assert f.restype is restype and list(f.argtypes) == argtypes, name                               # ... and typed at load
    assert lib.mi_abi_version() == 4          # additive: no signature of version 4 changed
    assert len(capi.Context._TIMES["scan_context"]) == 8
    for method in ("scan_context", "scan_context_search", "scan_context_times"):
        assert callable(getattr(capi.Context, method)), method
    assert callable(capi.scan_context_params) and callable(capi.scan_context_tables)
    assert callable(capi.scan_context_raw) and callable(capi.scan_context_search_raw)


def test_the_default_params_hold_the_documented_values(capi):
    p = capi.scan_context_params()
    assert [name for name, _ in capi.ScanContext.Params._fields_] == ["rings", "sectors", "max_radius", "z_offset", "reserved"]
    assert (p.rings, p.sectors, p.max_radius, p.z_offset) == (20, 60, 80.0, 2.0) and list(p.reserved) == [0] * 12
    assert C.sizeof(capi.ScanContext.Params) == 64
    q = capi.scan_context_params(rings=7, sectors=13, max_radius=12.5, z_offset=-1.0)
    assert (q.rings, q.sectors, q.max_radius, q.z_offset) == (7, 13, 12.5, -1.0)
    capi.lib().mi_scan_context_params_default(None)          # a null pointer is ignored


def test_the_compiler_agrees_with_the_params_layout(capi, tmp_path):
    cls, ctype = capi.ScanContext.Params, capi.ScanContext.C_TYPE
    out = ['#include <cstddef>', '#include "mi_slam.h"', 'static_assert(sizeof(%s) == %d, "%s: size");' % (ctype, C.sizeof(cls), ctype)]
    for field, ftype in cls._fields_:
        out.append('static_assert(offsetof(%s, %s) == %d, "%s.%s: offset");' % (ctype, field, getattr(cls, field).offset, ctype, field))
        out.append('static_assert(sizeof(%s::%s) == %d, "%s.%s: size");' % (ctype, field, C.sizeof(ftype), ctype, field))
    out.append("int main() { return 0; }")
    _compile(tmp_path, "scan_context_layout", "\n".join(out) + "\n")


def test_the_bindings_constants_are_read_from_the_kernels_header(capi):
    text = open(os.path.join(ROOT, "cuda-slam_amd", "csrc", "kernels.h")).read()
    for name in ("SC_SEARCH_CHUNK", "SC_SEARCH_WAVES", "SC_SLICE"):
        m = re.search(r"constexpr int %s = (\d+);" % name, text)
        assert m and int(m.group(1)) == getattr(capi, name), name
    assert capi.SC_SEARCH_CHUNK % capi.SC_SEARCH_WAVES == 0
    assert (capi.SCAN_CONTEXT_MAX_RINGS, capi.SCAN_CONTEXT_MAX_SECTORS, capi.SCAN_CONTEXT_MAX_ROWS) == (32, 64, 1 << 26)


def test_the_tables_call_refuses_without_writing(capi):
    edge2, dirs = np.full(40, -7.5), np.full(200, -7.5)
    good = capi.scan_context_params()
    lib = capi.lib()
    for kw, word in ((dict(rings=0), "rings"), (dict(rings=33), "rings"), (dict(sectors=0), "sectors"), (dict(sectors=65), "sectors"),
                     (dict(max_radius=0.0), "max_radius"), (dict(max_radius=-1.0), "max_radius"), (dict(max_radius=np.inf), "max_radius"),
                     (dict(max_radius=np.nan), "max_radius"), (dict(z_offset=np.nan), "z_offset"), (dict(z_offset=-np.inf), "z_offset")):
        bad = capi.scan_context_params(**kw)
        assert lib.mi_scan_context_tables(C.addressof(bad), edge2.ctypes.data, dirs.ctypes.data) == capi.MI_ERR_INVALID_ARG, kw
        msg = lib.mi_last_error().decode()
        assert msg.startswith("mi_scan_context_tables") and word in msg, msg
    for args in ((None, edge2.ctypes.data, dirs.ctypes.data), (C.addressof(good), None, dirs.ctypes.data), (C.addressof(good), edge2.ctypes.data, None)):
        assert lib.mi_scan_context_tables(*args) == capi.MI_ERR_INVALID_ARG
        assert lib.mi_last_error().decode().startswith("mi_scan_context_tables: null")
    assert (edge2 == -7.5).all() and (dirs == -7.5).all()


def test_a_null_context_is_refused_without_a_device(capi):
    params = capi.scan_context_params(rings=2, sectors=3)
    xyz, offsets = np.zeros((4, 3), np.float32), np.array([0, 4], np.int32)
    desc = np.full(6, -7.5, np.float32)
    rc = capi.scan_context_raw(None, xyz.ctypes.data, offsets.ctypes.data, 1, None, C.addressof(params), desc.ctypes.data)
    msg = capi.lib().mi_last_error().decode()
    assert rc == capi.MI_ERR_INVALID_ARG and msg.startswith("mi_scan_context: null context"), (rc, msg)
    assert (desc == -7.5).all()
    q, db = np.ones((1, 2, 3), np.float32), np.ones((2, 2, 3), np.float32)
    idx, shift, dist, second = np.full(1, -7, np.int32), np.full(1, -7, np.int32), np.full(1, -7.5, np.float32), np.full(1, -7.5, np.float32)
    rc = capi.scan_context_search_raw(None, q.ctypes.data, 1, db.ctypes.data, 2, None, C.addressof(params), idx.ctypes.data, dist.ctypes.data,
                                      shift.ctypes.data, second.ctypes.data)
    msg = capi.lib().mi_last_error().decode()
    assert rc == capi.MI_ERR_INVALID_ARG and msg.startswith("mi_scan_context_search: null context"), (rc, msg)
    assert idx[0] == -7 and shift[0] == -7 and dist[0] == -7.5 and second[0] == -7.5
    out = (C.c_double * 8)(*([-7.0] * 8))
    assert capi.lib().mi_scan_context_times(None, out) == capi.MI_ERR_INVALID_ARG and list(out) == [-7.0] * 8
    assert capi.lib().mi_last_error().decode().startswith("mi_scan_context_times")
