"""CPU suite: the pair features and bins of cuda-slam_amd/csrc/fpfh_pair.hpp, the arithmetic inside K18 of mi_fpfh_features, checked on the
host against the float64 restatement of tests/fpfh_reference.py.  tests/fpfh_pair_selftest.cpp includes the header alone; it is built as
a program of its own (no HIP runtime), plain and under the address and undefined-behaviour sanitizers, and run on a file of pairs.

Bounds: the bins are equal on every pair the restatement does not call fragile; the features agree within 1e-12 -- the fp64 chain is
about ten operations at unit magnitude, and atan2 may differ in its last bit between two libraries."""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import fpfh_reference as F
from conftest import ROOT

SOURCE = os.path.join(ROOT, "tests", "fpfh_pair_selftest.cpp")
BOUND = 1e-12


@functools.lru_cache(maxsize=None)
def catalogue():
    """float64 [m, 12]: p_i, n_i, p_j, n_j per pair, every number a float32"""
    rng = np.random.default_rng(201)
    m = 20000
    unit = lambda v: v / np.linalg.norm(v, axis=1, keepdims=True)
    p_i = rng.uniform(-1, 1, (m, 3))
    p_j = p_i + rng.normal(size=(m, 3)) * rng.choice([1e-3, 0.1, 1.0], (m, 1))
    n_i, n_j = unit(rng.normal(size=(m, 3))), unit(rng.normal(size=(m, 3)))
    n_j[: m // 4] = unit(n_i[: m // 4] + 0.1 * rng.normal(size=(m // 4, 3)))           # neighbours on a surface: nearly equal normals
    rows = [np.concatenate([p_i, n_i, p_j, n_j], axis=1)]
    p, q, z = [0.25, -0.5, 0.75], [1.25, -0.5, 0.75], [0.0, 0.0, 0.0]
    ex, ey, ez = [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]
    rows.append(np.array([
        p + ez + p + ey,                              # len 0
        p + ex + q + ex,                              # d parallel to both normals
        p + ex + q + ez,                              # d parallel to the normal at i (no swap, v = 0)
        p + ez + q + ex,                              # d parallel to the normal at j (swap, v = 0)
        p + z + q + ez,                               # a zero normal at i
        p + ez + q + z,                               # a zero normal at j
        p + z + q + z,                                # two zero normals
        p + ez + q + [0.0, 0.0, -1.0],                # opposite normals, both across d: theta = +-pi (fragile)
        p + ey + q + [0.0, -1.0, 0.0],
        p + [0.6, 0.0, 0.8] + q + [-0.6, 0.0, -0.8],  # opposite normals at an angle to d
        p + ez + q + ez,                              # equal normals across d: a tie of 0 and 0
        p + [0.6, 0.0, 0.8] + q + [0.6, 0.8, 0.0],    # a tie of |a1| and |a2| that is none of zeros (fragile)
        p + [0.0, 0.0, 3.0] + q + [0.0, 2.0, 2.0],    # normals that are not of unit length
    ], np.float64))
    out = np.concatenate(rows).astype(np.float32).astype(np.float64)
    out.setflags(write=False)
    return out


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]], ids=["plain", "sanitized"])
def test_pair_features_and_bins_against_the_restatement(tmp_path, flags):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "fpfh_pair_selftest")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off"] + flags + [SOURCE, "-o", exe])
    pairs = catalogue()
    path = str(tmp_path / "pairs.txt")
    np.savetxt(path, pairs, fmt="%.17g")
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rows = np.array([[float(x) for x in line.split()] for line in r.stdout.splitlines()])
    assert rows.shape == (len(pairs), 6), rows.shape
    feats, fragile = F.pair_features_and_fragility(pairs[:, 0:3], pairs[:, 3:6], pairs[:, 6:9], pairs[:, 9:12])
    fragile = fragile | F.near_an_edge(feats)
    assert np.isfinite(rows).all()
    # the degenerate pairs give (0, 0, 0) and bins 5 / 16 / 27, in both
    for row in range(len(pairs) - 13, len(pairs) - 6):
        assert (feats[row] == 0).all() and (rows[row, :3] == 0).all() and rows[row, 3:].tolist() == [5, 16, 27], row
    ok = ~fragile
    print("fpfh pairs: %d, %d fragile; features differ by at most %.3e" % (len(pairs), fragile.sum(), np.abs(rows[ok, :3] - feats[ok]).max()))
    assert fragile.sum() <= 0.001 * len(pairs)
    assert (np.abs(rows[ok, :3] - feats[ok]) <= BOUND).all()
    assert np.array_equal(rows[ok, 3:].astype(np.int64), F.bins(feats)[ok])
    assert (rows[:, 3] >= 0).all() and (rows[:, 3] <= 10).all() and (rows[:, 4] >= 11).all() and (rows[:, 4] <= 21).all() and (rows[:, 5] >= 22).all() and (rows[:, 5] <= 32).all()
