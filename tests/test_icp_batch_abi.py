"""CPU suite for the batched ICP entry points: the symbols exist and the binding lists them, the info struct has the header's layout,
mi_icp_batch_route is the pure function of sizes and rules the header promises, and without a device the call fails loudly."""
import ctypes as C

import numpy as np
import pytest


def test_library_and_binding_have_the_batched_entry_points(capi):
    lib = capi.lib()
    for name in ("mi_icp_batch_route", "mi_icp_register_batch"):
        assert hasattr(lib, name), name
        assert name in capi.EXPORTS, name
    assert lib.mi_abi_version() == 4          # additive: no signature of version 4 changed


def test_batch_info_layout(capi):
    assert C.sizeof(capi.IcpBatchInfo) == 32
    assert [f[0] for f in capi.IcpBatchInfo._fields_] == ["problems_batched", "problems_fallback", "launches", "reserved"]


def presets(capi):
    return [capi.icp_params(), capi.icp_params(cuda_slam=True)]


def test_route_covers_the_guaranteed_range(capi):
    rng = np.random.default_rng(42)
    pairs = [(1, 1), (1, 4096), (4096, 1), (4096, 4096), (4095, 4096), (64, 65), (2048, 2048)]
    pairs += [(int(a), int(b)) for a, b in rng.integers(1, 4097, (300, 2))]
    for p in presets(capi):
        for dist in (capi.DIST_CPU_ROUNDING, capi.DIST_FMA):
            for compose in (capi.COMPOSE_CPU_ADDITIVE, capi.COMPOSE_EXACT):
                p.dist_mode, p.compose_mode = dist, compose
                for n, m in pairs[:7]:
                    assert capi.icp_batch_route(n, m, p) == 1, (n, m)
        for n, m in pairs:
            assert capi.icp_batch_route(n, m, p) == 1, (n, m)
        for kw in (dict(filter_pairs=0), dict(filter_pairs=1), dict(abort_on_increase=1), dict(max_iterations=0), dict(max_iterations=7),
                   dict(sync_every=5), dict(nn_mode=capi.NN_GRID), dict(nn_mode=capi.NN_TREE), dict(nn_mode=capi.NN_BRUTEFORCE)):
            q = capi.icp_params(**kw)
            assert capi.icp_batch_route(4096, 4096, q) == 1, kw


def test_route_refuses_what_the_single_path_owns(capi):
    for p in presets(capi):
        assert capi.icp_batch_route(10 ** 6, 10 ** 6, p) == 0
    assert capi.icp_batch_route(100, 100, capi.icp_params(sum_mode=1)) == 0        # MI_SUM_CPU_SEQUENTIAL
    assert capi.icp_batch_route(100, 100, capi.icp_params(verbose=1)) == 0
    assert capi.icp_batch_route(0, 100, capi.icp_params()) == 0                    # not a problem at all
    assert capi.icp_batch_route(100, -1, capi.icp_params()) == 0


def test_route_is_monotone_in_both_sizes(capi):
    p = capi.icp_params()
    grid = [1, 2, 64, 1000, 4096, 4097, 5000, 8192, 10000, 16384, 20000, 65536, 10 ** 5, 10 ** 6]
    routed = {(n, m): capi.icp_batch_route(n, m, p) for n in grid for m in grid}
    for (n, m), r in routed.items():
        if r:
            assert all(routed[(n2, m2)] for n2 in grid for m2 in grid if n2 <= n and m2 <= m), (n, m)


def test_without_a_context_the_call_fails_loudly(capi):
    lib = capi.lib()
    p = capi.icp_params()
    pts = np.zeros((8, 3), np.float32)
    T = (C.c_float * 16)()
    it, err = C.c_int(0), C.c_float(0)
    lib.mi_icp_register.restype = C.c_int
    single = lib.mi_icp_register(None, pts.ctypes.data_as(C.POINTER(C.c_float)), 8, pts.ctypes.data_as(C.POINTER(C.c_float)), 8, C.byref(p), T,
                                 C.byref(it), C.byref(err))
    assert single != capi.MI_OK
    rng_ = np.array([[0, 8]], np.int32)
    Tb = np.zeros(16, np.float32)
    itb, why = np.zeros(1, np.int32), np.zeros(1, np.int32)
    eb = np.zeros(1, np.float32)
    info = capi.IcpBatchInfo()
    for n_problems in (1, 0):
        rc = capi.icp_register_batch_raw(None, n_problems, pts.ctypes.data, rng_.ctypes.data, pts.ctypes.data, rng_.ctypes.data, C.addressof(p),
                                         Tb.ctypes.data, itb.ctypes.data, eb.ctypes.data, why.ctypes.data, C.addressof(info))
        assert rc == single and rc != capi.MI_OK
        assert b"null context" in lib.mi_last_error()
