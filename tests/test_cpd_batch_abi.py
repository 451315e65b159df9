"""CPU suite for the batched CPD entry points: the symbols exist and the binding lists them, the info struct has the header's layout,
mi_cpd_batch_route is the pure, monotone function of sizes and rules the header promises, and without a context the call fails with the
single call's code and message."""
import ctypes as C
import itertools

import numpy as np


def test_library_and_binding_have_the_batched_entry_points(capi):
    lib = capi.lib()
    for name in ("mi_cpd_batch_route", "mi_cpd_register_batch"):
        assert hasattr(lib, name), name
        assert name in capi.EXPORTS, name
    assert lib.mi_abi_version() == 4          # additive: no signature of version 4 changed


def test_batch_info_layout(capi):
    assert C.sizeof(capi.CpdBatchInfo) == 32
    assert [f[0] for f in capi.CpdBatchInfo._fields_] == ["problems_batched", "problems_fallback", "launches", "reserved"]


def test_route_covers_the_guaranteed_range(capi):
    rng = np.random.default_rng(43)
    corners = [(1, 1), (1, 1024), (1024, 1), (1024, 1024)]
    pairs = corners + [(int(a), int(b)) for a, b in rng.integers(1, 1025, (300, 2))]
    p = capi.cpd_params()
    for m, n in pairs:
        assert capi.cpd_batch_route(m, n, p) == 1, (m, n)
    for const_scale, max_iterations, sync_every, sigma2_init in itertools.product((0, 1), (-1, 0, 7), (0, 1, 5), (0.0, 0.5)):
        q = capi.cpd_params(const_scale=const_scale, max_iterations=max_iterations, sync_every=sync_every, sigma2_init=sigma2_init)
        for m, n in pairs:
            assert capi.cpd_batch_route(m, n, q) == 1, (m, n, const_scale, max_iterations, sync_every, sigma2_init)
    # a given sigma^2_0 leaves the sigma2 mode nothing to compute
    assert capi.cpd_batch_route(1024, 1024, capi.cpd_params(sigma2_mode=capi.SIGMA2_CPU_SEQUENTIAL, sigma2_init=0.25)) == 1


def test_route_refuses_what_the_single_path_owns(capi):
    for kw in (dict(approximation=capi.CPD_APPROX_FULL), dict(approximation=capi.CPD_APPROX_HYBRID), dict(estep_mode=1),      # MI_ESTEP_CPU_SEQUENTIAL
               dict(sigma2_mode=capi.SIGMA2_CPU_SEQUENTIAL), dict(sigma2_mode=capi.SIGMA2_CPU_SEQUENTIAL, sigma2_init=-1.0), dict(verbose=1)):
        assert capi.cpd_batch_route(100, 100, capi.cpd_params(**kw)) == 0, kw
    p = capi.cpd_params()
    assert capi.cpd_batch_route(0, 100, p) == 0                    # not a problem at all
    assert capi.cpd_batch_route(100, 0, p) == 0
    assert capi.cpd_batch_route(-1, 100, p) == 0
    assert capi.cpd_batch_route(100, -1, p) == 0
    assert capi.cpd_batch_route(10 ** 6, 10 ** 6, p) == 0


def routing_edge(capi, p):
    n = 1
    while capi.cpd_batch_route(n, n, p):
        n += 1
        assert n < 10 ** 6
    return n - 1


def test_route_is_monotone_in_both_sizes(capi):
    p = capi.cpd_params()
    edge = routing_edge(capi, p)
    assert edge >= 1024
    grid = sorted({1, 2, 64, 1000, 1024, 1025, 2048, 2049, 4096, 4097, 8192, 20000, 10 ** 5, 10 ** 6, edge - 1, edge, edge + 1, 2 * edge})
    routed = {(m, n): capi.cpd_batch_route(m, n, p) for m in grid for n in grid}
    for (m, n), r in routed.items():
        if r:
            assert all(routed[(m2, n2)] for m2 in grid for n2 in grid if m2 <= m and n2 <= n), (m, n)
    assert routed[(edge, edge)] == 1 and routed[(edge + 1, 1)] == 0 and routed[(1, edge + 1)] == 0


def test_without_a_context_the_call_fails_as_the_single_call_does(capi):
    lib = capi.lib()
    p = capi.cpd_params(max_iterations=5)
    pts = np.zeros((8, 3), np.float32)
    fp = pts.ctypes.data_as(C.POINTER(C.c_float))
    T = (C.c_float * 16)()
    it, err, sc = C.c_int(0), C.c_float(0), C.c_float(0)
    lib.mi_cpd_register.restype = C.c_int
    lib.mi_last_error.restype = C.c_char_p
    single = lib.mi_cpd_register(None, fp, 8, fp, 8, C.byref(p), T, C.byref(sc), C.byref(it), C.byref(err))
    single_msg = lib.mi_last_error()
    assert single != capi.MI_OK and b"null context" in single_msg
    rng_ = np.array([[0, 8]], np.int32)
    Tb = np.zeros(16, np.float32)
    itb, why = np.zeros(1, np.int32), np.zeros(1, np.int32)
    eb, sb = np.zeros(1, np.float32), np.zeros(1, np.float32)
    info = capi.CpdBatchInfo()
    for n_problems in (1, 0):
        rc = capi.cpd_register_batch_raw(None, n_problems, pts.ctypes.data, rng_.ctypes.data, pts.ctypes.data, rng_.ctypes.data, C.addressof(p),
                                         Tb.ctypes.data, sb.ctypes.data, itb.ctypes.data, eb.ctypes.data, why.ctypes.data, C.addressof(info))
        assert rc == single
        assert lib.mi_last_error() == single_msg
