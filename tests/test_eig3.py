"""CPU suite: eig3_symmetric (cuda-slam_amd/csrc/eig3.hpp), the fp64 cyclic Jacobi solve behind mi_estimate_normals, checked on the host
against numpy.linalg.eigh.  tests/eig3_selftest.cpp includes the header alone; it is built as a program of its own (no HIP runtime), plain
and under the address and undefined-behaviour sanitizers, fed the catalogue below on stdin and run.

The bound 1e-13 (of the matrix's Frobenius norm; absolute for V^T V - I) is Jacobi's backward error, a few dozen 2^-53 for a handful of
sweeps of three rotations, with a margin of about ten."""
import functools
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

SOURCE = os.path.join(ROOT, "tests", "eig3_selftest.cpp")
BOUND = 1e-13


def sym(m):
    return (m + m.T) / 2.0


@functools.lru_cache(maxsize=None)
def catalogue():
    """(name, matrix) pairs; every matrix exactly symmetric"""
    rng = np.random.default_rng(61)
    cases = []
    for i in range(200):
        b = rng.normal(size=(3, 3))
        cases.append(("spd%d" % i, sym(b @ b.T + 1e-3 * np.eye(3))))
    cases.append(("zero", np.zeros((3, 3))))
    u, w = rng.normal(size=3), rng.normal(size=3)
    cases.append(("rank1", np.outer(u, u)))
    cases.append(("rank1_axis", np.outer([0.0, 2.0, 0.0], [0.0, 2.0, 0.0])))
    cases.append(("rank2", np.outer(u, u) + np.outer(w, w)))
    q = np.linalg.qr(rng.normal(size=(3, 3)))[0]
    for name, d in (("two_equal_low", (1.0, 1.0, 3.0)), ("two_equal_high", (1.0, 3.0, 3.0)), ("three_equal_rotated", (2.0, 2.0, 2.0))):
        cases.append((name, sym(q @ np.diag(d) @ q.T)))
    cases.append(("three_equal", 2.0 * np.eye(3)))
    cases.append(("two_equal_diagonal", np.diag([5.0, 1.0, 5.0])))
    for p in itertools.permutations((1.0, 2.0, 3.0)):
        cases.append(("diagonal_%d%d%d" % tuple(int(x) for x in p), np.diag(p)))
    cases.append(("indefinite", sym(rng.normal(size=(3, 3)))))
    for name, m in list(cases[:5]) + [("rank2", cases[203][1]), ("two_equal_low", cases[204][1])]:
        cases.append((name + "_x1e-30", m * 1e-30))
        cases.append((name + "_x1e+30", m * 1e+30))
    assert cases[203][0] == "rank2" and cases[204][0] == "two_equal_low"
    for _, m in cases:
        assert np.array_equal(m, m.T)
        m.setflags(write=False)
    return tuple(cases)


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]], ids=["plain", "sanitized"])
def test_eig3_symmetric_against_eigh(tmp_path, flags):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "eig3_selftest")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall"] + flags + [SOURCE, "-o", exe])
    cases = catalogue()
    text = "".join("%.17g %.17g %.17g %.17g %.17g %.17g\n" % (m[0, 0], m[0, 1], m[0, 2], m[1, 1], m[1, 2], m[2, 2]) for _, m in cases)
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rows = np.array([[float(x) for x in line.split()] for line in r.stdout.splitlines()])
    assert rows.shape == (len(cases), 12), rows.shape
    worst = [0.0, 0.0, 0.0]
    for (name, a), row in zip(cases, rows):
        lam, v = row[:3], row[3:].reshape(3, 3)
        assert np.isfinite(row).all(), name
        norm = float(np.linalg.norm(a))
        assert lam[0] <= lam[1] <= lam[2], (name, lam)
        want = np.linalg.eigh(a)[0]
        e_lam = np.abs(lam - want).max()
        e_res = max(np.linalg.norm(a @ v[:, i] - lam[i] * v[:, i]) for i in range(3))
        e_orth = np.linalg.norm(v.T @ v - np.eye(3))
        assert e_lam <= BOUND * norm, (name, e_lam, norm)
        assert e_res <= BOUND * norm, (name, e_res, norm)
        assert e_orth <= BOUND, (name, e_orth)
        if norm > 0:
            worst = [max(worst[0], e_lam / norm), max(worst[1], e_res / norm), max(worst[2], e_orth)]
    print("eig3 worst: eigenvalues %.2e, residual %.2e (of the Frobenius norm), orthogonality %.2e" % tuple(worst))
