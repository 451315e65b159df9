"""CPU suite: cuda-slam_amd/csrc/mls_fit.hpp, the frame, the basis, the fall-back decision and the projection behind mi_mls_smooth, checked
on the host.  tests/mls_fit_selftest.cpp includes the header alone; it is built as a program of its own (no HIP runtime), plain and under
the address and undefined-behaviour sanitizers, fed the catalogue below on stdin and run.

The bounds:
  frame          u . u - 1, v . v - 1, u . v, u . n, v . n: at most 8 x 2^-53 each (n is a unit vector to 2 x 2^-53; a cross product, a length and
                 three divisions follow); u_k = 0 exactly on the axis k the rule picks
  coefficients   a ball sampled from f = c . phi: | got - c | <= 1e-13 cond(S) | c |, S the normal equations scaled to a unit diagonal (numpy):
                 the bound tests/test_plane_solve.py holds plane_solve6 to
  whole fits     against tests/mls_reference.py on the same ball in the same order: the status equal, the smallest pivot within 1e-12, xyz
                 and the normal within 1e-11 radius / pivot (two eigen-solvers and two exp's a few 2^-53 apart, turned into the forward
                 error by the conditioning), the curvature within 1e-13
  fall-backs     order 1, five points, and a ball on a circle (1, a a, b b dependent), a line and a single spot: the plane, exactly q + o"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import knn_reference as K
import mls_reference as M
from conftest import ROOT

SOURCE = os.path.join(ROOT, "tests", "mls_fit_selftest.cpp")
U = 2.0 ** -53


def numbers(values):
    return " ".join("%.17g" % float(v) for v in np.asarray(values, np.float64).ravel())


def normals_catalogue():
    rng = np.random.default_rng(211)
    r2, r3 = np.sqrt(0.5), np.sqrt(1.0 / 3.0)
    fixed = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1),                      # along an axis: two zero components tie
             (r2, r2, 0), (r2, 0, r2), (0, r2, r2), (-r2, r2, 0), (r2, 0, -r2), (0, -r2, -r2),      # one zero; the other two tie
             (r3, r3, r3), (-r3, r3, -r3), (0.6, 0.6, np.sqrt(0.28)), (0.6, np.sqrt(0.28), 0.6), (np.sqrt(0.28), 0.6, 0.6)]
    rnd = rng.normal(size=(200, 3))
    rnd /= np.sqrt((rnd * rnd).sum(axis=1))[:, None]
    return np.concatenate([np.array(fixed, np.float64), rnd])


def coefficient_cases():
    """(n, o, s2, d [count, 3], the six coefficients, cond(S))"""
    rng = np.random.default_rng(223)
    cases = []
    for i in range(40):
        n = rng.normal(size=3)
        n /= np.sqrt((n * n).sum())
        (u,), (v,) = M.frame(n[None, :])
        o = 0.05 * rng.normal() * n
        coef = rng.normal(size=6) * np.array([0.1, 0.3, 0.3, 0.5, 0.5, 0.5])
        count = int(rng.integers(6, 60))
        ab = rng.uniform(-1, 1, (count, 2))
        a, b = ab[:, 0], ab[:, 1]
        phi = np.stack([np.ones(count), a, b, a * a, a * b, b * b], axis=1)
        f = phi @ coef
        d = o[None, :] + a[:, None] * u[None, :] + b[:, None] * v[None, :] + f[:, None] * n[None, :]
        s2 = float(rng.uniform(0.5, 2.0))
        w = np.exp(-(d * d).sum(axis=1) / s2)
        A = (phi * w[:, None]).T @ phi
        root = 1.0 / np.sqrt(np.diag(A))
        cases.append((n, o, s2, d, coef, float(np.linalg.cond(A * root[:, None] * root[None, :]))))
    return cases


def fit_cases():
    """(name, order, radius, the query float32 [3], the cloud float32 [count, 3]) -- the ball is the whole cloud"""
    rng = np.random.default_rng(227)
    cases = []
    for i in range(30):
        count = int(rng.integers(6, 80))
        xy = rng.uniform(-1, 1, (count, 2))
        z = 0.3 * np.sin(1.3 * xy[:, 0]) * np.cos(1.1 * xy[:, 1]) + 0.01 * rng.normal(size=count)
        cloud = (np.concatenate([xy, z[:, None]], axis=1) + rng.normal(size=3) * (10.0 if i % 3 == 0 else 0.0)).astype(np.float32)
        cases.append(("surface%d" % i, 2, 8.0, cloud[0] if i % 2 else (cloud[0] + np.float32(0.05)).astype(np.float32), cloud))
    cloud = cases[0][4]
    cases.append(("order1", 1, 8.0, cloud[3], cloud))
    cases.append(("five_points", 2, 8.0, cloud[1], cloud[:5]))
    t = np.arange(12) * (2 * np.pi / 12)
    circle = np.stack([np.cos(t), np.sin(t), np.zeros(12)], axis=1).astype(np.float32)
    cases.append(("circle", 2, 8.0, np.array([0, 0, 0.1], np.float32), circle))
    line = np.stack([np.arange(9), 2.0 * np.arange(9), np.zeros(9)], axis=1).astype(np.float32)
    cases.append(("line", 2, 40.0, line[4], line))
    cases.append(("spot", 2, 1.0, np.array([1.5, -2.25, 3.0], np.float32), np.tile(np.array([[1.5, -2.25, 3.0]], np.float32), (9, 1))))
    return cases


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]], ids=["plain", "sanitized"])
def test_mls_fit_header(tmp_path, flags):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "mls_fit_selftest")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off"] + flags + [SOURCE, "-o", exe])
    normals, coefs, fits = normals_catalogue(), coefficient_cases(), fit_cases()
    text = "".join("f %s\n" % numbers(n) for n in normals)
    text += "".join("c %s %s %.17g %d %s\n" % (numbers(n), numbers(o), s2, len(d), numbers(d)) for n, o, s2, d, _, _ in coefs)
    for _, order, radius, q, cloud in fits:
        s = float(np.float32(radius))
        text += "q %d %.17g %s %d %s\n" % (order, s * s, numbers(q), len(cloud), numbers(cloud.astype(np.float64) - q.astype(np.float64)))
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [[float(x) for x in line.split()] for line in r.stdout.splitlines()]
    assert len(lines) == len(normals) + len(coefs) + len(fits)

    # ---- the frame
    worst = 0.0
    for n, row in zip(normals, lines):
        u, v = np.array(row[:3]), np.array(row[3:])
        k = int(np.argmin(np.abs(n)))                                    # (the lowest axis of a tie)
        assert u[k] == 0.0, (n, u)
        err = max(abs(u @ u - 1), abs(v @ v - 1), abs(u @ v), abs(u @ n), abs(v @ n))
        worst = max(worst, err / U)
        assert err <= 8 * U, (n, err / U)
        (ru,), (rv,) = M.frame(n[None, :])
        assert np.abs(u - ru).max() <= 4 * U and np.abs(v - rv).max() <= 4 * U, n          # the restatement's frame is this one
    print("frame: worst departure from orthonormal %.2f x 2^-53 over %d normals" % (worst, len(normals)))

    # ---- a ball sampled from f = c . phi gives c back
    worst = 0.0
    for (n, o, s2, d, coef, cond), row in zip(coefs, lines[len(normals):]):
        assert row[0] == 1.0 and row[1] >= 1e-10, (cond, row[:2])
        err, bound = np.linalg.norm(np.array(row[2:]) - coef), 1e-13 * cond * np.linalg.norm(coef)
        worst = max(worst, err / bound)
        assert err <= bound, (err, bound, cond)
    print("coefficients: worst error / bound %.3f over %d balls" % (worst, len(coefs)))

    # ---- whole fits against the restatement, the fall-backs among them
    for (name, order, radius, q, cloud), row in zip(fits, lines[len(normals) + len(coefs):]):
        ref = M.smooth(cloud, radius, K.DIST_CPU_ROUNDING, queries=q[None, :], order=order)
        assert ref["neighbours"][0] == len(cloud), name
        status, pivot, xyz, normal, n, o, curv = int(row[0]), row[1], np.array(row[2:5]), np.array(row[5:8]), np.array(row[8:11]), np.array(row[11:14]), row[14]
        assert status == ref["status"][0], (name, status, pivot, ref["pivot"][0])
        sign = 1.0 if normal @ ref["normals64"][0] >= 0 else -1.0
        assert abs(curv - float(ref["curvature"][0])) <= 6e-8 * curv + 1e-13, name
        if name.startswith("surface"):
            assert status == M.QUADRATIC and pivot >= 1e-4 and abs(pivot - ref["pivot"][0]) <= 1e-12, (name, pivot, ref["pivot"][0])
            bound = 1e-11 * float(np.float32(radius)) / pivot
            assert np.abs(xyz - ref["xyz64"][0]).max() <= bound and np.abs(normal - sign * ref["normals64"][0]).max() <= bound, name
        else:
            assert status == M.PLANE, name
            assert np.array_equal(xyz, q.astype(np.float64) + o) and np.array_equal(normal, n), name           # exactly the plane's projection
            assert np.isfinite(xyz).all() and np.isfinite(normal).all() and abs(normal @ normal - 1) <= 4 * U, name
            if name in ("order1", "five_points", "circle"):
                assert np.abs(xyz - ref["xyz64"][0]).max() <= 1e-12 and np.abs(normal - sign * ref["normals64"][0]).max() <= 1e-12, name
            if name == "circle":                                             # the query above the circle's plane comes down onto it
                assert abs(xyz[2]) <= 1e-15 and np.abs(xyz[:2]).max() <= 1e-15, (pivot, xyz)
            if name in ("circle", "line"):
                assert pivot < 1e-10, (name, pivot)                              # (a rounding's worth, of either sign)
            if name == "spot":                                                   # an unusable diagonal entry: a a sums to nothing
                assert pivot == 0.0 and np.array_equal(xyz, q.astype(np.float64)) and curv == 0.0, (name, pivot)
