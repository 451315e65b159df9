"""CPU suite: the Fast Global Registration entry points exist with the header's prototypes, mi_fgr_params_default gives the header's defaults,
a NULL context is refused without a device with every output untouched (the refusals that need a context: tests/test_gpu_fgr.py), the
schedule header is held to its rule by a host program of its own, and the restatement the GPU tests use as their oracle
(tests/fgr_reference.py) gives the answers worked by hand: the mu schedule at k = 0, 3, 4, 7 and 8 with its stop at delta^2, a two-match
linearisation, the used list with and without the tuple filter, and the library's summation order on integers."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import fgr_reference as F
from conftest import ROOT
from test_capi_prototypes import _compile


def test_library_exports_the_fgr_entry_points(capi):
    lib = capi.lib()
    protos = {p[0]: p for p in capi._PROTOTYPES}
    for name, nargs in (("mi_fgr_register", 16), ("mi_fgr_tuples", 11), ("mi_fgr_system", 12), ("mi_fgr_register_times", 2), ("mi_fgr_params_default", 1)):
        assert hasattr(lib, name) and name in capi.EXPORTS, name
        assert len(protos[name][4]) == nargs, (name, protos[name][2])
    assert protos["mi_fgr_system"][4][8] is C.c_int and protos["mi_fgr_register"][4][2] is C.c_int and protos["mi_fgr_register"][3] is C.c_int
    assert lib.mi_abi_version() == 4          # additive: no signature of version 4 changed
    text = open(capi._HEADER).read()
    assert "#define MI_FGR_MAX_TUPLES (1 << 20)" in text and "#define MI_FGR_STAGES 8" in text
    assert capi.FGR_MAX_TUPLES == 1 << 20 and 3 * capi.FGR_MAX_TUPLES > 65536
    for name in ("fgr_register", "fgr_tuples", "fgr_system", "fgr_register_times"):
        assert callable(getattr(capi.Context, name))


def test_the_compiler_agrees_with_the_params_layout(capi, tmp_path):
    cls, ctype = capi.Fgr.Params, capi.Fgr.C_TYPE
    out = ['#include <cstddef>', '#include "mi_slam.h"', 'static_assert(sizeof(%s) == %d, "%s: size");' % (ctype, C.sizeof(cls), ctype)]
    for field, ftype in cls._fields_:
        out.append('static_assert(offsetof(%s, %s) == %d, "%s.%s: offset");' % (ctype, field, getattr(cls, field).offset, ctype, field))
        out.append('static_assert(sizeof(%s::%s) == %d, "%s.%s: size");' % (ctype, field, C.sizeof(ftype), ctype, field))
    out.append("int main() { return 0; }")
    _compile(tmp_path, "fgr_layout", "\n".join(out) + "\n")


def test_params_default(capi):
    p = capi.Fgr.Params()
    C.memset(C.addressof(p), 0xFF, C.sizeof(p))
    capi.lib().mi_fgr_params_default(C.byref(p))
    assert p.max_distance == 0.0 and p.division_factor == np.float32(1.4) and p.decrease_every == 4 and p.max_iterations == 64
    assert p.tuple_scale == np.float32(0.95) and p.max_tuples == 1000 and p.tuple_trials == 0 and p.seed == 0
    assert p.eps_rotation == 0.0 and p.eps_translation == 0.0 and p.sync_every == 0 and p.verbose == 0 and list(p.reserved) == [0] * 8
    capi.lib().mi_fgr_params_default(None)                            # a NULL struct is ignored
    q = capi.fgr_params(0.02, tuple_scale=0.5, seed=2 ** 64 - 1)
    assert q.max_distance == np.float32(0.02) and q.tuple_scale == 0.5 and q.seed == 2 ** 64 - 1 and q.max_tuples == 1000
    with pytest.raises(TypeError):
        capi.fgr_params(0.02, hypotheses=3)
    assert capi.fgr_used_capacity(q, 65) == 3000 and capi.fgr_used_capacity(capi.fgr_params(1.0, tuple_scale=0.0), 65) == 65
    assert capi.fgr_used_capacity(capi.fgr_params(1.0, tuple_trials=7), 65) == 21


def test_a_null_context_is_refused_without_a_device(capi):
    cloud, idx, p = np.zeros((4, 3), np.float32), np.arange(4, dtype=np.int32), capi.fgr_params(0.1)
    T, w, us, ut = np.full(16, -7, np.float32), np.full(12, -7, np.float32), np.full(12, -7, np.int32), np.full(12, -7, np.int32)
    it, why, used, acc, err, mu = C.c_int(-7), C.c_int(-7), C.c_int(-7), C.c_int(-7), C.c_float(-7), C.c_float(-7)
    rc = capi.fgr_register_raw(None, cloud.ctypes.data, 4, cloud.ctypes.data, 4, idx.ctypes.data, C.addressof(p), None, T.ctypes.data, C.addressof(it),
                               C.addressof(err), C.addressof(why), C.addressof(used), C.addressof(mu), w.ctypes.data, us.ctypes.data)
    msg = capi.lib().mi_last_error().decode()
    assert rc == capi.MI_ERR_INVALID_ARG and msg.startswith("mi_fgr_register:") and "null context" in msg
    assert (T == -7).all() and (w == -7).all() and (us == -7).all() and [it.value, why.value, used.value, err.value, mu.value] == [-7] * 5
    rc = capi.fgr_tuples_raw(None, cloud.ctypes.data, 4, cloud.ctypes.data, 4, idx.ctypes.data, C.addressof(p), C.addressof(used), us.ctypes.data,
                             ut.ctypes.data, C.addressof(acc))
    msg = capi.lib().mi_last_error().decode()
    assert rc == capi.MI_ERR_INVALID_ARG and msg.startswith("mi_fgr_tuples:") and "null context" in msg
    assert (us == -7).all() and (ut == -7).all() and used.value == -7 and acc.value == -7
    sums, centre, mu64 = np.full(32, -7.0), np.full(3, -7, np.float32), C.c_double(-7)
    rc = capi.fgr_system_raw(None, cloud.ctypes.data, 4, cloud.ctypes.data, 4, idx.ctypes.data, C.addressof(p), None, 0, sums.ctypes.data,
                             centre.ctypes.data, C.addressof(mu64))
    msg = capi.lib().mi_last_error().decode()
    assert rc == capi.MI_ERR_INVALID_ARG and msg.startswith("mi_fgr_system:") and "null context" in msg
    assert (sums == -7).all() and (centre == -7).all() and mu64.value == -7
    out = (C.c_double * 8)(*([-7.0] * 8))
    assert capi.lib().mi_fgr_register_times(None, out) == capi.MI_ERR_INVALID_ARG and list(out) == [-7.0] * 8
    assert capi.lib().mi_last_error().decode().startswith("mi_fgr_register_times")


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]], ids=["plain", "sanitized"])
def test_schedule_header_keeps_its_rule(tmp_path, flags):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "fgr_schedule_selftest")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off"] + flags + [os.path.join(ROOT, "tests", "fgr_schedule_selftest.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "fgr_schedule selftest ok" in r.stdout, r.stdout + r.stderr


def test_restatement_of_the_schedule_worked_by_hand():
    # D2 = 16, delta = 1.5 (delta^2 = 2.25), factor 2, every 4 updates: 16 at k = 0 .. 3, 8 at 4 .. 7, 4 at 8 .. 11, 2 at 12 .. 15 -- at or
    # below delta^2 = 2.25, so the division stops there: 2 for every later k.  All exact in binary.
    for k, want in ((0, 16.0), (3, 16.0), (4, 8.0), (7, 8.0), (8, 4.0), (11, 4.0), (12, 2.0), (16, 2.0), (400, 2.0)):
        assert F.mu_at(16.0, 1.5, 2.0, 4, k) == want, k
    # mu exactly AT delta^2 is not divided ("if mu > delta^2"): delta = 2 stops at 4
    assert [F.mu_at(16.0, 2.0, 2.0, 4, k) for k in (7, 8, 12, 99)] == [8.0, 4.0, 4.0, 4.0]
    # decrease_every = 1 divides at every update; the factor is the fp32 value promoted: 1.4f, not 1.4
    assert F.mu_at(16.0, 1.5, 2.0, 1, 3) == 2.0
    assert F.mu_at(1.0, 1e-3, 1.4, 4, 4) == 1.0 / float(np.float32(1.4)) != 1.0 / 1.4
    # the scale: fp32 bounds, fp64 extents
    box = np.array([[0, 0, 0], [3, 4, 12], [1, 1, 1]], np.float32)
    assert F.diagonal2(box) == 169.0 and F.scale2(box, 0.5 * box) == 169.0 and F.scale2(0.5 * box, 2 * box) == 676.0


def test_restatement_of_a_two_match_linearisation_worked_by_hand():
    # c0 = (0, 0, 0) (the target box is symmetric), identity pose, mu = 3:
    #   match 0: p = (1, 2, 2), q = (1, 2, 0)  -> r = (0, 0, 2),  d2 = 4, w = 3 / 7,   u = (1, 2, 2)
    #   match 1: p = (-1, -2, 0), q = (-1, -2, 0) -> r = 0,       d2 = 0, w = 1, l = 1, u = (-1, -2, 0)
    p = np.array([[1, 2, 2], [-1, -2, 0]], np.float64)
    q = np.array([[1, 2, 0], [-1, -2, 0]], np.float64)
    T = F.terms(p, q, np.eye(3), np.zeros(3), np.zeros(3), 3.0)
    w0 = 3.0 / 7.0
    l0 = w0 * w0
    # H(0, 0) = l (u_z^2 + u_y^2): rows J_y[0] = -u_z, J_z[0] = u_y
    assert T[0, 0] == l0 * ((0.0 + 4.0) + 4.0) and T[1, 0] == 1.0 * ((0.0 + 0.0) + 4.0)
    # H(0, 1) = l (-u_x u_y): J_z[0] J_z[1] = u_y * -u_x
    assert T[0, 1] == l0 * -2.0 and T[1, 1] == -2.0
    # H(0, 4) = l (-u_z), H(0, 5) = l u_y, H(3, 3) = H(4, 4) = H(5, 5) = l, H(3, 4) = 0
    k = {(i, j): n for n, (i, j) in enumerate((i, j) for i in range(6) for j in range(i, 6))}
    assert T[0, k[0, 4]] == l0 * -2.0 and T[0, k[0, 5]] == l0 * 2.0 and T[0, k[3, 4]] == 0.0
    assert [T[0, k[i, i]] for i in (3, 4, 5)] == [l0] * 3 and [T[1, k[i, i]] for i in (3, 4, 5)] == [1.0] * 3
    # g = l J^T r with r = (0, 0, 2): g_0 = l u_y r_z = 4 l, g_1 = l (-u_x) r_z = -2 l, g_2 = 0, g_5 = 2 l
    assert T[0, 21:27].tolist() == [l0 * 4.0, l0 * -2.0, 0.0, 0.0, 0.0, l0 * 2.0] and not T[1, 21:27].any()
    # e = l d2 + mu (w - 1)^2, aux = d2, count = 1, the last two entries 0
    assert T[0, 27] == l0 * 4.0 + 3.0 * ((w0 - 1.0) * (w0 - 1.0)) and T[1, 27] == 0.0
    assert T[:, 28].tolist() == [4.0, 0.0] and T[:, 29].tolist() == [1.0, 1.0] and not T[:, 30:].any()
    # e is the Geman-McClure value mu d2 / (mu + d2) = 12 / 7 to rounding
    assert abs(T[0, 27] - 12.0 / 7.0) <= 4 * F.U * 12.0 / 7.0
    # a pose that carries x to infinity or NaN: the term is zeros, count included
    for bad in (np.inf, np.nan):
        Tb = F.terms(p, q, np.eye(3), np.array([bad, 0.0, 0.0]), np.zeros(3), 3.0)
        assert not Tb.any()
    # the whole system through the used list: sums = both terms added, the weights are l
    src, tgt = p.astype(np.float32), np.concatenate([q, -q]).astype(np.float32)         # the target box is symmetric: c0 = 0
    used = dict(used_src=np.array([0, 1]), used_tgt=np.array([0, 1]))
    sy = F.system(src, tgt, used, mu=3.0)
    assert (sy["centre"] == 0).all() and np.array_equal(sy["sums"], T[0] + T[1]) and np.array_equal(sy["fsum"][:30], (T[0] + T[1])[:30])


def test_restatement_of_the_used_list():
    src, tgt, idx, R0, t0, true = F.planted(65, 0.3, seed=4, unmatched=5)
    plain = F.used_list(src, tgt, idx, tuple_scale=0.0)
    assert plain["used_src"].tolist() == list(range(65)) and plain["used_tgt"].tolist() == list(range(65)) and plain["accepted"] == 0
    got = F.used_list(src, tgt, idx, tuple_scale=0.95, max_tuples=10, seed=9)
    assert got["trials"] == 6500 and got["accepted"] > 10 and len(got["used_src"]) == 30
    more = F.used_list(src, tgt, idx, tuple_scale=0.95, max_tuples=20, seed=9)
    assert more["accepted"] == got["accepted"] and more["used_src"][:30].tolist() == got["used_src"].tolist()     # max_tuples only cuts
    # a tuple of three TRUE matches always passes a rigid pair of clouds at 0.95 (noise 0.002 on edges of about 0.5): most kept ones are true
    assert true[got["used_src"]].mean() > 0.8
    # a kept tuple's three matches are distinct, and its edges pass the rule both ways
    s, t = src[got["used_src"]].astype(np.float64).reshape(-1, 3, 3), tgt[got["used_tgt"]].astype(np.float64).reshape(-1, 3, 3)
    e2 = float(np.float32(0.95)) ** 2
    for a, b in ((0, 1), (1, 2), (0, 2)):
        ls, lt = ((s[:, a] - s[:, b]) ** 2).sum(axis=1), ((t[:, a] - t[:, b]) ** 2).sum(axis=1)
        assert (ls >= e2 * lt * (1 - 1e-12)).all() and (lt >= e2 * ls * (1 - 1e-12)).all() and (ls > 0).all()
    # source and target scaled apart: no trial passes
    none = F.used_list(src, 3 * tgt, idx, tuple_scale=0.95, seed=9)
    assert none["accepted"] == 0 and len(none["used_src"]) == 0


def test_restatement_of_the_summation_order_on_integers():
    # integers up to 2^20 add exactly in any order: the fixed order gives the plain sum at every size class (one row, several rows, the slabs)
    rng = np.random.default_rng(3)
    for used in (1, 63, 64, 65, 200, 70000):
        T = rng.integers(-2 ** 20, 2 ** 20, (used, 32)).astype(np.float64)
        assert np.array_equal(F.device_order_sums(T), T.sum(axis=0)), used
    assert F.tree_depth(64) == 6 + 1 + 8 and F.tree_depth(65536) == 6 + 128 + 8 and F.tree_depth(70000) == 6 + (3 + 8) + (8 + 8)
    # and on one row of doubles it is the halving tree, not the left-to-right sum
    # lanes 1 and 33 meet first (2^-53 + 2^-53 = 2^-52) and reach lane 0's 1 together; added one by one each would be rounded away
    v = np.zeros((64, 32))
    v[0, 0], v[1, 0], v[33, 0] = 1.0, 2.0 ** -53, 2.0 ** -53
    assert F.device_order_sums(v)[0] == 1.0 + 2.0 ** -52 and (1.0 + 2.0 ** -53) + 2.0 ** -53 == 1.0
