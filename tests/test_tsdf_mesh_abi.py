"""CPU suite: mi_tsdf_mesh exists -- the header declares it and points at its numpy twin, the library exports it, the binding types it from
the header -- the interface version has not moved, the table's header carries the kernels' constants, and a null context is refused without
a device and with every output untouched."""
import ctypes as C
import os
import re

import numpy as np

from conftest import ROOT

V, I, F, L = C.c_void_p, C.c_int, C.c_float, C.c_longlong


def test_the_header_declares_the_mesh_call():
    text = open(os.path.join(ROOT, "include", "mi_slam.h")).read()
    assert re.search(r"\bint mi_tsdf_mesh\s*\(", text)
    assert "tests/tsdf_mesh_reference.py" in text and "tools/gen_mc_table.py" in text
    assert "#define MI_TSDF_STAGES 8" in text
    flat = " ".join(re.sub(r"/\*.*?\*/", " ", text, flags=re.S).split())
    assert ("int mi_tsdf_mesh(mi_ctx* ctx, const int* coord, const float* tsdf, const float* weight, int nv, const float origin3[3], float voxel_size, "
            "float min_weight , float* out_xyz, float* out_normals , long long vertex_capacity, long long* out_nvert, int* out_tri , "
            "long long tri_capacity, long long* out_ntri);") in flat


def test_the_library_exports_the_mesh_call(capi):
    lib = capi.lib()
    protos = {p[0]: p for p in capi._PROTOTYPES}
    name, argtypes = "mi_tsdf_mesh", [V, V, V, V, I, V, F, F, V, V, L, V, V, L, V]
    assert hasattr(lib, name) and name in capi.EXPORTS
    f = getattr(lib, name)
    assert protos[name][3] is I and protos[name][4] == argtypes, protos[name][2]       # read from the header ...
    assert f.restype is I and list(f.argtypes) == argtypes                             # ... and typed at load
    assert lib.mi_abi_version() == 4          # additive: no signature of version 4 changed
    assert callable(capi.Context.tsdf_mesh) and callable(capi.tsdf_mesh_raw)
    assert len(capi.Context._TIMES["tsdf"]) == 8


def test_the_tables_header_and_the_kernels_agree():
    table = open(os.path.join(ROOT, "cuda-slam_amd", "csrc", "tsdf_mesh_table.hpp")).read()
    kernels = open(os.path.join(ROOT, "cuda-slam_amd", "csrc", "kernels.h")).read()
    cases = int(re.search(r"constexpr int TSDF_MESH_CASES = (\d+);", table).group(1))
    block = int(re.search(r"constexpr int TSDF_BLOCK = (\d+);", kernels).group(1))
    assert cases == block == 256              # a workgroup stages one row of the table per lane
    assert int(re.search(r"constexpr int TSDF_MESH_MAX_TRIANGLES = (\d+);", table).group(1)) == 5
    for k in ("K76 tsdf_mesh_classify", "K77 tsdf_mesh_edges", "K78 tsdf_mesh_triangles"):
        assert k in kernels, k


def test_a_null_context_is_refused_without_a_device(capi):
    origin = np.zeros(3, np.float32)
    one = (np.zeros((1, 3), np.int32), np.zeros(1, np.float32), np.ones(1, np.float32))
    xyz, nrm, tri = np.full((3, 3), -7.5, np.float32), np.full((3, 3), -7.5, np.float32), np.full((3, 3), -7, np.int32)
    nvert, ntri = C.c_longlong(-7), C.c_longlong(-7)
    rc = capi.tsdf_mesh_raw(None, one[0].ctypes.data, one[1].ctypes.data, one[2].ctypes.data, 1, origin.ctypes.data, 0.5, 1.0, xyz.ctypes.data,
                            nrm.ctypes.data, 3, C.addressof(nvert), tri.ctypes.data, 3, C.addressof(ntri))
    msg = capi.lib().mi_last_error().decode()
    assert rc == capi.MI_ERR_INVALID_ARG and msg.startswith("mi_tsdf_mesh: null context"), (rc, msg)
    assert nvert.value == -7 and ntri.value == -7 and (xyz == -7.5).all() and (nrm == -7.5).all() and (tri == -7).all()
