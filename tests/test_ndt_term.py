"""CPU suite: the term of one (point, voxel) pair of cuda-slam_amd/csrc/ndt_term.hpp, the arithmetic inside the step kernel of
mi_ndt_register, checked on the host.  tests/ndt_term_selftest.cpp includes the header alone; it is built as a program of its own (no HIP
runtime), plain and under the address and undefined-behaviour sanitizers, and run on a file of 10 000 random pairs and the no-term cases.

Bounds: d, Md and m are the same IEEE operations in the header, in the program's plain-C restatement and in tests/ndt_reference.py, so they
are equal bit for bit; e and w pass through one exp, which two libraries may round differently: 2 units of the last place."""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import ndt_reference as N
from conftest import ROOT

SOURCE = os.path.join(ROOT, "tests", "ndt_term_selftest.cpp")
RANDOM = 10000


@functools.lru_cache(maxsize=None)
def catalogue():
    """float64 [m, 14]: q, mu, M, h, k per pair; q, mu and M are float32 values"""
    rng = np.random.default_rng(311)
    mu = rng.uniform(-50, 50, (RANDOM, 3))
    q = mu + rng.normal(size=(RANDOM, 3)) * rng.choice([1e-3, 0.1, 1.0], (RANDOM, 1))
    B = rng.normal(size=(RANDOM, 3, 3))
    S = B @ B.transpose(0, 2, 1) + 1e-3 * np.eye(3)                                    # positive definite
    M = np.stack([S[:, a, b] for a, b in N.TRI], axis=1) * rng.choice([0.1, 1.0, 100.0], (RANDOM, 1))
    hk = np.tile(N.constants(0.5)[2:], (RANDOM, 1))
    hk[RANDOM // 2:] = N.constants(2.0, 0.3)[2:]
    rows = np.concatenate([q, mu, M, hk], axis=1)
    h, k = N.constants(1.0)[2:]
    special = np.array([
        [1, 2, 3, 1, 2, 3.5, 0, 0, 0, 0, 0, 0, h, k],                # zero matrix: no distribution
        [1, 2, 3, 1, 2, 3.5, -1, 0, 0, -1, 0, -1, h, k],             # negative definite: m < 0
        [1, 2, 3, 1, 2, 3.5, np.nan, 0, 0, 1, 0, 1, h, k],           # NaN
        [1e18, 0, 0, -1e18, 0, 0, 1e18, 0, 0, 1e18, 0, 1e18, h, k],  # m finite but huge: e = 0, still a term
        [1, 0, 0, 0, 0, 0, np.inf, 0, 0, 1, 0, 1, h, k],             # an infinite entry: m is not finite, no term
        [1, 2, 3, 1, 2, 3, 1, 0, 0, 1, 0, 1, h, k],                  # d = 0: m = 0, e = 1
        [1, 2, 3, 1, 2, 3.5, 0, 0, 0, 0, 0, 4, h, k],                # a singular matrix that is not zero
    ], np.float64)
    out = np.concatenate([rows, special])
    out[:, :12] = out[:, :12].astype(np.float32).astype(np.float64)
    out.setflags(write=False)
    return out


def ulps(a, b):
    return np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]], ids=["plain", "sanitized"])
def test_terms_against_the_plain_restatement_and_numpy(tmp_path, flags):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "ndt_term_selftest")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off"] + flags + [SOURCE, "-o", exe])
    pairs = catalogue()
    path = str(tmp_path / "pairs.txt")
    np.savetxt(path, pairs, fmt="%.17g")
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()
    rows = np.array([[float(x) for x in line.split()] for line in lines[:-1]])
    assert rows.shape == (len(pairs), 20), rows.shape
    got, plain = rows[:, :10], rows[:, 10:]
    ref = N.term(pairs[:, 0:3], pairs[:, 3:6], pairs[:, 6:12], pairs[:, 12], pairs[:, 13])
    # which pairs have a term: the same in all three; the special rows as their comments say
    assert np.array_equal(got[:, 0], plain[:, 0]) and np.array_equal(got[:, 0] == 1, ref["ok"])
    assert got[:RANDOM, 0].all() and got[RANDOM:, 0].tolist() == [0, 0, 0, 1, 0, 1, 1]
    ok = ref["ok"]
    exact = np.concatenate([ref["d"], ref["Md"], ref["m"][:, None]], axis=1)
    assert np.array_equal(got[ok, 1:8], plain[ok, 1:8]) and np.array_equal(got[ok, 1:8], exact[ok])
    assert (got[~ok] == 0).all()
    worst = max(ulps(got[ok, 8], ref["e"][ok]).max(), ulps(got[ok, 9], ref["w"][ok]).max(), ulps(got[ok, 8], plain[ok, 8]).max())
    print("ndt terms: %d with a term; e and w differ by at most %.2f units of the last place" % (ok.sum(), worst))
    assert worst <= 2
    assert got[RANDOM + 3, 8] == 0 and got[RANDOM + 5, 7] == 0 and got[RANDOM + 5, 8] == 1
    # a decreasing weight: along every random pair's own matrix, the term with the larger m has the smaller w
    order = np.argsort(got[:RANDOM // 2, 7])
    assert (np.diff(got[:RANDOM // 2, 9][order]) <= 0).all()
    # the fold of every term into one point's sums, against the plain restatement's: the same operations in the same order
    fold = [float(x) for x in lines[-1].split()]
    assert len(fold) == 22 and fold[:11] == fold[11:] and fold[10] == ok.sum()
