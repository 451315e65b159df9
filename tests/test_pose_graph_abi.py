"""CPU suite: the pose-graph entry points exist -- the header declares them, the params struct and MI_POSE_GRAPH_STAGES, the library exports
them, the binding types them from the header -- the interface version has not moved, the default params hold the documented values, and a
null context is refused without a device and with every output untouched."""
import ctypes as C
import os
import re

import numpy as np

from conftest import ROOT
from test_capi_prototypes import _compile

NAMES = ("mi_pose_graph_default_params", "mi_pose_graph_optimize", "mi_pose_graph_system", "mi_pose_graph_times")


def test_the_header_declares_the_pose_graph_interface():
    text = open(os.path.join(ROOT, "include", "mi_slam.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, text), name
    assert re.search(r"typedef struct mi_pose_graph_params \{.*?\} mi_pose_graph_params;", text, re.S)
    assert re.search(r"#define MI_POSE_GRAPH_STAGES 8\b", text)


def test_library_exports_the_pose_graph_entry_points(capi):
    lib = capi.lib()
    V, I = C.c_void_p, C.c_int
    for name, restype, argtypes in (("mi_pose_graph_default_params", None, [V]),
                                    ("mi_pose_graph_optimize", C.c_int, [V, V, I, V, V, V, V, V, I, V, V, V, V, V]),
                                    ("mi_pose_graph_system", C.c_int, [V, V, I, V, V, V, V, V, I, V, V, I] + [V] * 11),
                                    ("mi_pose_graph_times", C.c_int, [V, V])):
        assert hasattr(lib, name), name
        assert name in capi.EXPORTS, name
        f = getattr(lib, name)
        assert f.restype is restype and list(f.argtypes) == argtypes, name
    assert lib.mi_abi_version() == 4          # additive: no signature of version 4 changed
    assert len(capi.Context._TIMES["pose_graph"]) == 8
    for method in ("pose_graph_optimize", "pose_graph_system", "pose_graph_times"):
        assert callable(getattr(capi.Context, method)), method


def test_the_default_params_hold_the_documented_values(capi):
    p = capi.pose_graph_params()
    got = [getattr(p, name) for name, _ in capi.PoseGraph.Params._fields_]
    assert [name for name, _ in capi.PoseGraph.Params._fields_] == ["max_iterations", "max_pcg_iterations", "reference_node", "pcg_tolerance",
                                                                   "relative_decrease", "absolute_cost", "lambda0", "line_process_mu"]
    assert got == [50, 200, 0, 1e-8, 1e-9, 0.0, 1e-6, 0.0], got


def test_the_compiler_agrees_with_the_params_layout(capi, tmp_path):
    cls, ctype = capi.PoseGraph.Params, capi.PoseGraph.C_TYPE
    out = ['#include <cstddef>', '#include "mi_slam.h"', 'static_assert(sizeof(%s) == %d, "%s: size");' % (ctype, C.sizeof(cls), ctype)]
    for field, ftype in cls._fields_:
        out.append('static_assert(offsetof(%s, %s) == %d, "%s.%s: offset");' % (ctype, field, getattr(cls, field).offset, ctype, field))
        out.append('static_assert(sizeof(%s::%s) == %d, "%s.%s: size");' % (ctype, field, C.sizeof(ftype), ctype, field))
    out.append("int main() { return 0; }")
    _compile(tmp_path, "pose_graph_layout", "\n".join(out) + "\n")


def test_a_null_context_is_refused_without_a_device(capi):
    poses = np.tile(np.eye(4).reshape(16), (2, 1))
    src, tgt = np.array([0], np.int32), np.array([1], np.int32)
    Z, info = np.eye(4).reshape(1, 16).copy(), np.eye(6).reshape(1, 36).copy()
    params = capi.pose_graph_params()
    out, w, chi2, report = np.full((2, 16), -7.5), np.full(1, -7.5), np.full(1, -7.5), np.full(8, -7.5)
    rc = capi.pose_graph_optimize_raw(None, poses.ctypes.data, 2, src.ctypes.data, tgt.ctypes.data, Z.ctypes.data, info.ctypes.data, None, 1,
                                      C.addressof(params), out.ctypes.data, w.ctypes.data, chi2.ctypes.data, report.ctypes.data)
    msg = capi.lib().mi_last_error().decode()
    assert rc == capi.MI_ERR_INVALID_ARG and msg.startswith("mi_pose_graph_optimize: null context"), (rc, msg)
    assert (out == -7.5).all() and (w == -7.5).all() and (chi2 == -7.5).all() and (report == -7.5).all()
    outs = [np.full(n, -7.5) for n in (6, 1, 1, 21, 6, 42, 12, 12, 12, 2, 1)]
    rc = capi.pose_graph_system_raw(None, poses.ctypes.data, 2, src.ctypes.data, tgt.ctypes.data, Z.ctypes.data, info.ctypes.data, None, 1,
                                    C.addressof(params), None, 1, *[o.ctypes.data for o in outs])
    msg = capi.lib().mi_last_error().decode()
    assert rc == capi.MI_ERR_INVALID_ARG and msg.startswith("mi_pose_graph_system: null context"), (rc, msg)
    assert all((o == -7.5).all() for o in outs)


def test_the_times_call_refuses_null(capi):
    out = (C.c_double * 8)(*([-7.0] * 8))
    assert capi.lib().mi_pose_graph_times(None, out) == capi.MI_ERR_INVALID_ARG and list(out) == [-7.0] * 8
    assert capi.lib().mi_last_error().decode().startswith("mi_pose_graph_times")
