"""CPU suite: the k-NN entry points exist, the argument errors that need no device are refused, and the restatement the GPU tests use
as their oracle (tests/knn_reference.py) agrees with the committed C oracle for k = 1, bit for bit in both distance arithmetics, and
with answers worked by hand on a 3 x 3 x 3 integer lattice."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import knn_reference as K


def test_library_exports_the_knn_entry_points(capi):
    lib = capi.lib()
    for name in ("mi_knn_search", "mi_knn_search_times"):
        assert hasattr(lib, name), name
        assert name in capi.EXPORTS, name
    assert lib.mi_abi_version() == 4          # additive: no signature of version 4 changed
    assert capi.KNN_MAX_K == 32


def test_a_null_context_is_refused_without_a_device(capi):
    cloud = np.zeros((4, 3), np.float32)
    idx = np.full((4, 2), -7, np.int32)
    rc = capi.knn_search_raw(None, cloud.ctypes.data, 4, cloud.ctypes.data, 4, 2, capi.DIST_FMA, float("inf"), idx.ctypes.data, None, None)
    assert rc == capi.MI_ERR_INVALID_ARG and "null context" in capi.lib().mi_last_error().decode()
    assert (idx == -7).all()
    out = (C.c_double * 8)()
    f = capi.lib().mi_knn_search_times
    f.argtypes, f.restype = [C.c_void_p, C.c_void_p], C.c_int
    assert f(None, out) == capi.MI_ERR_INVALID_ARG


@pytest.mark.parametrize("mode", [K.DIST_CPU_ROUNDING, K.DIST_FMA])
@pytest.mark.parametrize("scale", [1.0, 100.0])
@pytest.mark.parametrize("seed", [3, 4])
def test_restatement_is_the_oracle_search_for_k_1(oracle, mode, scale, seed):
    rng = np.random.default_rng(seed)
    q = (rng.uniform(-5, 5, (1000, 3)) * scale).astype(np.float32)
    c = (rng.uniform(-5, 5, (1500, 3)) * scale).astype(np.float32)
    c[700:800] = c[:100]                                   # duplicates: the lower index wins
    q[:50] = c[200:250]                                    # exact hits
    ridx, rd2 = oracle.nn_search(q, c, dist_mode=mode)
    idx, d2, count = K.knn(q, c, 1, mode)
    assert np.array_equal(idx[:, 0], ridx) and np.array_equal(d2[:, 0].view(np.uint32), rd2.view(np.uint32))
    assert (count == 1).all()


def test_the_two_arithmetics_differ_often_enough_to_tell_them_apart():
    rng = np.random.default_rng(5)
    q = rng.uniform(-5, 5, (500, 3)).astype(np.float32)
    c = rng.uniform(-5, 5, (1000, 3)).astype(np.float32)
    a, b = K.sorted_keys(q, c, K.DIST_CPU_ROUNDING, keep=16), K.sorted_keys(q, c, K.DIST_FMA, keep=16)
    assert (a != b).any(axis=1).mean() > 0.5


def nearest_f32(s):
    """The float32 nearest to the rational s (ties to even), by exact comparison."""
    mid = np.float32(float(s))
    cands = [np.nextafter(mid, np.float32(-np.inf)), mid, np.nextafter(mid, np.float32(np.inf))]
    return min(cands, key=lambda v: (abs(Fraction(float(v)) - s), int(v.view(np.uint32)) & 1))


def test_fma_emulation_rounds_once():
    # a * a = 1 + 2^-11 + 2^-24 is the midpoint of two float32 neighbours; + 2^-80 lies above it by less than a float64 can hold: a
    # float64 add followed by a cast rounds to even (down), the one correct rounding goes up
    a = np.array([1.0 + 2.0 ** -12], np.float32)
    c = np.array([2.0 ** -80], np.float32)
    assert np.float32(np.float64(a[0]) * np.float64(a[0]) + np.float64(c[0])) == np.float32(1 + 2.0 ** -11)
    assert K.fma_sq_f32(a, c)[0] == np.float32(1 + 2.0 ** -11 + 2.0 ** -23)
    assert K.fma_sq_f32(-a, -c)[0] == np.float32(1 + 2.0 ** -11)            # (below the midpoint)
    rng = np.random.default_rng(9)
    a = (rng.uniform(-10, 10, 2000) * 10.0 ** rng.integers(-3, 4, 2000)).astype(np.float32)
    c = (rng.uniform(0, 100, 2000) * 10.0 ** rng.integers(-6, 4, 2000)).astype(np.float32)
    got = K.fma_sq_f32(a, c)
    for i in range(2000):
        assert got[i] == nearest_f32(Fraction(float(a[i])) ** 2 + Fraction(float(c[i]))), i


def lattice3():
    g = np.arange(3, dtype=np.float32)
    z, y, x = np.meshgrid(g, g, g, indexing="ij")
    return np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1)       # index = x + 3 y + 9 z


@pytest.mark.parametrize("mode", [K.DIST_CPU_ROUNDING, K.DIST_FMA])
def test_restatement_on_a_lattice_worked_by_hand(mode):
    L = lattice3()
    # the centre point: itself, then its six face neighbours at distance 1 in index order
    idx, d2, count = K.knn(np.array([[1, 1, 1]], np.float32), L, 7, mode)
    assert idx[0].tolist() == [13, 4, 10, 12, 14, 16, 22] and d2[0].tolist() == [0, 1, 1, 1, 1, 1, 1] and count[0] == 7
    # the centre of the first cell: its eight corners, all at 0.75, in index order
    idx, d2, count = K.knn(np.array([[0.5, 0.5, 0.5]], np.float32), L, 8, mode)
    assert idx[0].tolist() == [0, 1, 3, 4, 9, 10, 12, 13] and (d2[0] == 0.75).all() and count[0] == 8
    # self mode drops the point itself (by index) and keeps its duplicate, at +0
    L2 = np.concatenate([L, L[13:14]])
    idx, d2, count = K.knn(None, L2, 3, mode)
    assert idx[13].tolist() == [27, 4, 10] and d2[13].tolist() == [0, 1, 1] and np.signbit(d2[13, 0]) == False   # noqa: E712
    assert idx[27].tolist() == [13, 4, 10]
    assert 0 not in idx[0].tolist() and idx[0].tolist() == [1, 3, 9]
    # fewer points than k: padded with (-1, +inf)
    idx, d2, count = K.knn(np.array([[0, 0, 0]], np.float32), L[:3], 5, mode)
    assert idx[0].tolist() == [0, 1, 2, -1, -1] and d2[0].tolist() == [0, 1, 4, np.inf, np.inf] and count[0] == 3
    idx, d2, count = K.knn(None, L[:3], 5, mode)
    assert idx[1].tolist() == [0, 2, -1, -1, -1] and count.tolist() == [2, 2, 2]
    # the distance limit cuts (a candidate AT the limit exists), and count agrees
    q = np.array([[1, 1, 1]], np.float32)
    for limit, want in ((0.0, 1), (0.5, 1), (1.0, 7), (1.5, 7), (2.0, 19), (3.0, 27)):
        idx, d2, count = K.knn(q, L, 27, mode, max_d2=limit)
        assert count[0] == want and (idx[0, want:] == -1).all() and np.isinf(d2[0, want:]).all() and (d2[0, :want] <= limit).all()
