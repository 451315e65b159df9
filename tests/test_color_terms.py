"""CPU suite: the arithmetic of cuda-slam_amd/csrc/color_terms.hpp, what K48 and K49 of the colored ICP compute per point and per pair,
checked on the host against the float64 restatement of tests/color_reference.py, bit for bit.  tests/color_terms_selftest.cpp includes the
header alone; it is built as a program of its own (no HIP runtime), plain and under the address and undefined-behaviour sanitizers, with
-ffp-contract=off as the library is, and run on files of operands written with 17 significant digits (an exact round trip).

Bit for bit is the right bound: both sides are the same IEEE float64 operations in the same order, and neither may fuse any."""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import color_reference as CR
from conftest import ROOT

SOURCE = os.path.join(ROOT, "tests", "color_terms_selftest.cpp")
FLAGS = {"plain": [], "sanitized": ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]}


@functools.lru_cache(maxsize=None)
def program(kind):
    import tempfile
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = os.path.join(tempfile.mkdtemp(prefix="color_terms_"), "color_terms_selftest_" + kind)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off"] + FLAGS[kind] + [SOURCE, "-o", exe])
    return exe


def run(kind, mode, rows, tmp_path):
    path = str(tmp_path / (mode + ".txt"))
    np.savetxt(path, rows, fmt="%.17g")
    r = subprocess.run([program(kind), mode, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = np.array([[float(x) for x in line.split()] for line in r.stdout.splitlines()])
    assert len(out) == len(rows), out.shape
    return out


def f32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float64).view(np.uint64), np.ascontiguousarray(b, np.float64).view(np.uint64))


@pytest.mark.parametrize("kind", sorted(FLAGS))
def test_pair_entries_bit_for_bit(tmp_path, kind):
    rng = np.random.default_rng(311)
    m = 1000
    unit = lambda v: v / np.linalg.norm(v, axis=1, keepdims=True)
    q = rng.uniform(-3, 3, (m, 3)) + rng.choice([0.0, 100.0], (m, 1))
    a = q + rng.normal(size=(m, 3)) * rng.choice([1e-3, 0.1], (m, 1))
    c0 = q.mean(axis=0)[None, :] + np.zeros((m, 3))
    n, g = unit(rng.normal(size=(m, 3))), rng.normal(size=(m, 3)) * rng.choice([0.0, 0.3, 5.0], (m, 1))
    Ia, Ib = rng.uniform(0, 1, m), rng.uniform(0, 1, m)
    lam = rng.choice([0.0, 0.5, 0.968, 1.0], m)
    rows = f32(np.concatenate([q, a, c0, n, g, Ia[:, None], Ib[:, None], lam[:, None]], axis=1))
    got = run(kind, "pairs", rows, tmp_path)
    assert got.shape == (m, 28)
    for value in np.unique(rows[:, 17]):
        pick = rows[:, 17] == value
        r = rows[pick]
        JG, JC, rG, rC = CR.pair_terms(r[:, 0:3], r[:, 3:6], r[:, 6:9], r[:, 9:12], r[:, 12:15], r[:, 15], r[:, 16])
        want = CR.pair_entries(JG, JC, rG, rC, value)
        assert same_bits(got[pick], want), (kind, value, np.abs(got[pick] - want).max())
        if value == 1.0:      # the geometric terms alone, up to the sign of a zero
            plane = np.stack([JG[:, i] * JG[:, j] for i in range(6) for j in range(i, 6)] + [JG[:, i] * rG for i in range(6)] + [rG * rG], axis=1)
            assert (want == plane).all()


@pytest.mark.parametrize("kind", sorted(FLAGS))
def test_gradient_solve_bit_for_bit(tmp_path, kind):
    rng = np.random.default_rng(312)
    m = 1000
    B = rng.normal(size=(m, 3, 3)) * rng.choice([1e-3, 1.0, 30.0], (m, 1, 1))
    A = B @ B.transpose(0, 2, 1)                                       # positive definite, whatever the scale ...
    A[-60:-40] = -A[-60:-40]                                           # ... a negative determinant ...
    A[-40:-20, 2, :] = A[-40:-20, 0, :]
    A[-40:-20, :, 2] = A[-40:-20, :, 0]
    A[-40:-20, 2, 2] = A[-40:-20, 0, 0]                                # ... two equal rows and columns ...
    A[-20:] = np.round(A[-20:])
    A[-20:, 1] = 2 * A[-20:, 0]
    A[-20:, :, 1] = 2 * A[-20:, :, 0]
    A[-20:, 1, 1] = 4 * A[-20:, 0, 0]                                  # ... and small integers with an exactly zero determinant
    M = np.stack([A[:, 0, 0], A[:, 0, 1], A[:, 0, 2], A[:, 1, 1], A[:, 1, 2], A[:, 2, 2]], axis=1)
    b = rng.normal(size=(m, 3))
    got = run(kind, "solve", np.concatenate([M, b], axis=1), tmp_path)
    d, det = CR.solve_gradient(M, b)
    ok = (det > 0) & np.isfinite(det)
    assert np.array_equal(got[:, 3] == 1, ok) and 20 <= (~ok).sum() <= 60 and not ok[-20:].any() and not ok[-60:-40].any()
    assert same_bits(got[:, :3], d), (kind, np.abs(got[:, :3] - d).max())
    assert (got[~ok, :3] == 0).all()
    # the restatement's own error on the well-conditioned part, against numpy's solve
    good = ok & (CR.cond1(M) < 1e6)
    x = np.linalg.solve(CR.full3(M[good]), b[good][:, :, None])[:, :, 0]
    assert good.sum() > 500 and (np.abs(d[good] - x) <= 1e-9 * np.abs(x).max(axis=1, keepdims=True)).all()


@pytest.mark.parametrize("kind", sorted(FLAGS))
def test_normal_equations_bit_for_bit(tmp_path, kind):
    rng = np.random.default_rng(313)
    m = 1000
    n = rng.normal(size=(m, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    n[:10] = 0
    e = rng.normal(size=(m, 5, 3)) * 0.05
    delta = rng.normal(size=(m, 5)) * 0.1
    rows = f32(np.concatenate([n, np.concatenate([e, delta[:, :, None]], axis=2).reshape(m, 20)], axis=1))
    got = run(kind, "sums", rows, tmp_path)
    nb = rows[:, 3:].reshape(m, 5, 4)
    M, b = CR.normal_equations(rows[:, :3], nb[:, :, :3], nb[:, :, 3], np.full(m, 5))
    assert same_bits(got[:, :6], M) and same_bits(got[:, 6:], b)
