"""CPU suite: the CPD drivers' host plan (cuda-slam_amd/csrc/cpd_plan.hpp) -- chunk plans, rows of partial sums, the FGT's cell count and
constants, the route of an approximated E-step, the monomial tables.  tests/cpd_plan_selftest.cpp includes the header alone; it is built as a
program of its own (no HIP), plain and under the address and undefined-behaviour sanitizers, and run: it asserts the rounding rules itself and
prints one line per case, which is compared here, for equality, with the Python restatements the float64 E-step tests rest on
(estep_reference.plan_chunks / plan, fgt_reference.cluster_count / ndi / hsigma_inv / pd_of / exponents) and with what mi_fgt_tables returns."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import estep_reference as E
import fgt_reference as F
from conftest import ROOT

SOURCE = os.path.join(ROOT, "tests", "cpd_plan_selftest.cpp")
SIZES = (1, 2, 63, 64, 65, 2047, 2048, 2049, 4096, 100000, 1000000)
FGT_SIZES = ((2, 2), (400, 500), (700, 300), (35947, 35947))
ORDERS = (1, 2, 8, 16)


def _f32(word):
    return np.array([int(word, 16)], np.uint32).view(np.float32)[0]


def _bits(value):
    return int(np.array([value], np.float32).view(np.uint32)[0])


@pytest.fixture(scope="module", params=[[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]], ids=["plain", "sanitized"])
def lines(request, tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("cpd_plan") / "cpd_plan_selftest")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off"] + request.param + [SOURCE, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "cpd plan selftest ok" in r.stdout, r.stdout[-4000:] + r.stderr[-4000:]
    out = {}
    for line in r.stdout.splitlines():
        key, _, rest = line.partition(" ")
        out.setdefault(key, []).append(rest.split())
    return out


def test_chunk_plans_are_the_python_restatement(lines):
    got = {tuple(int(v) for v in row[:3]): [int(v) for v in row[3:]] for row in lines["chunks"]}
    assert sorted(got) == sorted((cu, m, n) for cu in (1, 256, 304) for m in SIZES for n in SIZES)
    for (cu, m, n), row in got.items():
        p = E.plan(m, n, cu)
        assert row == [p["k_chunks"], p["k_chunk_len"], p["x_chunks"], p["x_chunk_len"], p["tiles_m"], p["tiles_n"]], (cu, m, n)
        assert tuple(row[0:2]) == E.plan_chunks(n, 4, m, cu) and tuple(row[2:4]) == E.plan_chunks(m, 2, n, cu), (cu, m, n)


def test_fgt_constants_are_the_python_restatement(lines):
    cells = {(int(r[0]), int(r[1]), r[2], r[3]): r[4:] for r in lines["cells"]}
    want = [(m, n, s2, s0) for m, n in FGT_SIZES for s2 in (2.0, 0.3, 0.05, 1e-4) for s0 in (1.0, 50.0)]
    assert len(cells) == len(want)
    for m, n, s2, s0 in want:
        K, h = cells[m, n, "%08x" % _bits(s2), "%08x" % _bits(s0)]
        assert int(K) == F.cluster_count(m, n, s2, s0), (m, n, s2, s0)
        assert int(h, 16) == _bits(F.hsigma_inv(s2)[0]), (m, n, s2)
    ndi = {(int(r[0]), int(r[1]), r[2], r[3]): r[4] for r in lines["ndi"]}
    assert len(ndi) == len(FGT_SIZES) * 4 * len(F.WEIGHTS)
    for (m, n, s2w, ww), word in ndi.items():
        assert int(word, 16) == _bits(F.ndi(_f32(s2w), _f32(ww), m, n)), (m, n, _f32(s2w), _f32(ww))
    assert sorted(_bits(w) for w in F.WEIGHTS) == sorted({int(k[3], 16) for k in ndi})


def test_monomial_tables_are_the_library_s_and_the_restatement_s(lines, capi, oracle):
    assert [(int(p), int(pd)) for p, pd in lines["pd"]] == [(p, F.pd_of(p)) for p in ORDERS]
    for p in ORDERS:
        rows = [r for r in lines["table"] if int(r[0]) == p]
        assert [int(r[1]) for r in rows] == list(range(F.pd_of(p)))
        mono = np.array([int(r[2]) for r in rows], np.uint32)
        ck = np.array([int(r[3], 16) for r in rows], np.uint32)
        slot = np.array([int(r[4]) for r in rows], np.int32)
        exps = np.stack([mono & 0xff, (mono >> 8) & 0xff, (mono >> 16) & 0xff], axis=1).astype(np.int64)
        lib_exps, lib_ck, lib_slot = capi.fgt_tables(p)                           # mi_fgt_tables: the same function, through the library
        assert np.array_equal(exps, lib_exps) and np.array_equal(ck, lib_ck.view(np.uint32)) and np.array_equal(slot, lib_slot)
        assert np.array_equal(exps, F.exponents(p))                               # fgt.cpp's graded recursion, written out
        assert np.array_equal(ck, oracle.fgt_ck(p).view(np.uint32))               # ComputeC_k's step-by-step rounding
