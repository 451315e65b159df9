"""CPU suite: the 3 x 3 Kabsch solve (cuda-slam_amd/csrc/svd3.hpp kabsch_rotation) compiled for the host, where it is the IEEE form,
on the seeded matrix catalogue of tests/kabsch_catalogue.py.

It must retrace the oracle (oracle_kabsch_from_h, Eigen's JacobiSVD restated) bit for bit: R, the singular values and det(U V^T).  The
device's IEEE form is held to the same bits (tests/test_gpu_kabsch3.py), and where R is not a continuous function of H the fast form
hands the matrix to the IEEE one -- so these bits are what every path returns there."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT, check_measured
from kabsch_catalogue import EPS, catalogue, kabsch64, objective_deficit, orthogonality, posedness

HARNESS = r"""
#include "svd3.hpp"
extern "C" void host_kabsch(const float* h, int count, float* r, float* s, float* det)
{
    for (int i = 0; i < count; i++) {
        mislam::Mat3 H;
        for (int k = 0; k < 9; k++) H.a[k / 3][k % 3] = h[9 * i + k];
        const mislam::Kabsch3 q = mislam::kabsch_rotation<false>(H);
        for (int k = 0; k < 9; k++) r[9 * i + k] = q.R.a[k / 3][k % 3];
        for (int k = 0; k < 3; k++) s[3 * i + k] = q.S[k];
        det[i] = q.det;
    }
}
"""


@pytest.fixture(scope="module")
def host_kabsch(tmp_path_factory):
    """svd3.hpp's host form as a shared library (hipcc, host code only: no device is needed; no contraction, like the oracle)."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    d = tmp_path_factory.mktemp("kabsch3")
    src, so = d / "harness.cpp", d / "libkabsch3.so"
    src.write_text(HARNESS)
    subprocess.check_call([hipcc, "-x", "hip", "--offload-host-only", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
                           "-I", os.path.join(ROOT, "cuda-slam_amd", "csrc"), str(src), "-o", str(so)])
    lib = C.CDLL(str(so))
    fp = C.POINTER(C.c_float)

    def run(H):
        H = np.ascontiguousarray(H, np.float32)
        n = H.shape[0]
        R, S, det = np.empty((n, 3, 3), np.float32), np.empty((n, 3), np.float32), np.empty(n, np.float32)
        lib.host_kabsch(H.ctypes.data_as(fp), n, R.ctypes.data_as(fp), S.ctypes.data_as(fp), det.ctypes.data_as(fp))
        return R, S, det
    return run


def oracle_all(oracle, H):
    out = [oracle.kabsch_from_h(h) for h in H]
    return (np.stack([o[0] for o in out]), np.stack([o[2] for o in out]), np.array([o[3] for o in out], np.float32))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_host_form_is_the_oracle_bit_for_bit(host_kabsch, oracle):
    H, names = catalogue()
    R, S, det = host_kabsch(H)
    Ro, So, deto = oracle_all(oracle, H)
    for what, a, b in (("R", R, Ro), ("S", S, So), ("det", det, deto)):
        differ = ~(bits(a) == bits(b)).reshape(len(H), -1).all(axis=1)
        assert not differ.any(), "%s differs from the oracle on %d matrices, classes %s" % (what, differ.sum(), sorted(set(names[differ])))
    assert np.isfinite(R).all() and np.isfinite(S).all()


def test_host_form_against_float64(host_kabsch):
    H, names = catalogue()
    R, S, det = host_kabsch(H)
    R64, S64, d, g = kabsch64(H)
    cond, well, ill = posedness(S64, g)
    # the catalogue reaches both sides: the exact reflections and the det < 0 ties up to a 1e-5 gap are ill-posed, the 1e-2 ties well-posed
    assert well.sum() > 2800 and ill.sum() > 700
    assert ill[names == "reflection"].all()
    for gap in ("0", "1e-07", "1e-05"):
        assert ill[names == "tie_det_neg_" + gap].all()
    assert well[names == "tie_det_neg_0.01"].all()
    ratio = np.abs(R.astype(np.float64) - R64).max(axis=(1, 2)) / (cond + EPS)
    worst = int(np.argmax(np.where(well, ratio, 0)))
    print("host IEEE form vs float64 Kabsch: worst ratio %.3f (%s)" % (ratio[worst], names[worst]))
    check_measured("kabsch3_host_ieee_vs_f64_ratio", ratio[well].max(), 32.0)
    # singular values: backward stable, so within a few eps * sigma_1 of float64
    assert (np.abs(S - S64) <= 8 * EPS * S64[:, :1]).all()
    # every matrix, well-posed or not: near-orthogonal, det +1, and the Kabsch objective at its maximum
    e, de = orthogonality(R)
    print("host IEEE form: max |R^T R - I| %.2e, |det R - 1| %.2e (eps %.2e)" % (e.max(), de.max(), EPS))
    assert e.max() <= 64 * EPS and de.max() <= 64 * EPS, (e.max(), de.max())     # (measured: 41 eps and 32 eps; Jacobi sweeps do not re-orthonormalise)
    assert objective_deficit(R, H, S64, d).max() <= 16 * EPS
