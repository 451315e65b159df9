"""CPU suite: cuda-slam_amd/csrc/tsdf_cast.hpp, the arithmetic of mi_tsdf_raycast, checked on the host.  tests/tsdf_cast_selftest.cpp includes
the header alone; it is built as a program of its own (no HIP runtime, nothing of HIP on the include path), plain and under the address and
undefined-behaviour sanitizers, and run: once on its own facts, and once over a small fused map read from a file this test writes, where
a ray's direction, the voxel of every sample, the end of the march, r and which field gave it, depth, point and normal are compared with
tests/tsdf_raycast_reference.py bit for bit -- and the march with empty-space skipping with the march that visits every sample."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import tsdf_raycast_reference as RC
import tsdf_reference as R
from conftest import ROOT

SOURCE = os.path.join(ROOT, "tests", "tsdf_cast_selftest.cpp")
RECORD = np.dtype([("d", "<f8", 3), ("r", "<f8"), ("end_k", "<i4"), ("trilinear", "<i4"), ("hit", "<i4"), ("same_with_skip", "<i4"),
                   ("depth", "<u4"), ("xyz", "<u4", 3), ("normal", "<u4", 3), ("pad", "<u4")])


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def yawed(yaw, pitch, t):
    cy, sy, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    T = np.eye(4)
    T[:3, :3] = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1]]) @ np.array([[cp, 0, sp], [0, 1, 0], [-sp, 0, cp]])
    T[:3, 3] = t
    return T.astype(np.float32)


@pytest.fixture(scope="module", params=[[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]], ids=["plain", "sanitized"])
def selftest(request, tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("tsdf_cast") / "tsdf_cast_selftest")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off"] + request.param + [SOURCE, "-o", exe])
    return exe


def test_tsdf_casts_keep_their_contract(selftest):
    r = subprocess.run([selftest], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "tsdf_cast selftest ok" in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("shift,skipping", [(0.0, 1), (3e4, 1), (2e6, 0)], ids=["at-the-origin", "shifted-3e4", "shifted-2e6"])
def test_the_header_casts_as_the_reference_does(selftest, tmp_path, shift, skipping):
    # a sphere of radius 2 fused from its centre and a little off it (so some voxels have weight 2), seen from a posed sensor inside; the
    # lattice, the sphere and the sensor shifted together, to where fp32 positions are as coarse as 0.002 and 0.25 against a voxel of 0.1
    rng = np.random.default_rng(11)
    ball = rng.normal(size=(1500, 3))
    ball = (2 * ball / np.linalg.norm(ball, axis=1)[:, None]).astype(np.float32)
    move = np.array([shift, -shift, shift / 2], np.float32)
    origin = (np.full(3, -3, np.float32) + move).astype(np.float32)
    centre = np.eye(4, dtype=np.float32)
    centre[:3, 3] = move
    off = centre.copy()
    off[:3, 3] += np.array([0.3, -0.2, 0.1], np.float32)
    m = R.integrate([ball, (ball.astype(np.float64) - [0.3, -0.2, 0.1]).astype(np.float32)], [centre, off], origin, 0.1, 0.3)
    pose = yawed(0.4, -0.2, move.astype(np.float64) + [0.2, 0.1, -0.3])
    dirs = rng.normal(size=(300, 3)).astype(np.float32) * rng.uniform(0.1, 5, (300, 1)).astype(np.float32)
    dirs[7] = 0                                                   # no length: a miss
    voxel, min_weight, min_range, max_range = np.float32(0.1), np.float32(2.0 if shift == 0 else 1.0), np.float32(0.25), np.float32(4.0)

    depth, xyz, nrm, hits, info = RC.raycast(m, origin, voxel, max_range, pose, dirs, min_weight=min_weight, min_range=min_range, details=True)
    K = info["K"]
    assert 0 < hits < len(dirs) or shift == 2e6

    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as fh:
        fh.write(np.array([len(m[0]), len(dirs), 1, 0], "<i4").tobytes())
        fh.write(np.concatenate([origin, [voxel, min_weight, min_range, max_range, 0]]).astype("<f4").tobytes())
        fh.write(np.ascontiguousarray(pose.T, "<f4").tobytes())                 # column-major
        for a, t in ((m[0], "<i4"), (m[1], "<f4"), (m[2], "<f4"), (dirs, "<f4")):
            fh.write(np.ascontiguousarray(a, t).tobytes())
    r = subprocess.run([selftest, src, dst], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = open(dst, "rb").read()
    head = np.frombuffer(raw, "<i4", 4)
    assert head[0] == K and head[1] == skipping, (head, K, r.stdout)
    per_ray = np.dtype([("rec", RECORD), ("voxels", "<i4", (K, 4))])
    got = np.frombuffer(raw, per_ray, len(dirs), offset=16)
    rec = got["rec"]

    live = info["d"].any(axis=1)
    assert not live[7] and np.array_equal(rec["d"].view(np.uint64), info["d"].view(np.uint64)), "directions"
    o = pose[:3, 3].astype(np.float64)
    for k in range(K):                                            # the voxel of every sample of every live ray
        c, ok = RC.sample_voxels(o, info["d"], np.float64(min_range) + np.float64(k) * (np.float64(voxel) / 2), origin, voxel)
        assert np.array_equal(got["voxels"][live, k, 0] != 0, ok[live]) and np.array_equal(got["voxels"][live, k, 1:][ok[live]], c[live][ok[live]]), "sample %d" % k
    assert np.array_equal(rec["end_k"], info["end_k"]), "where the march ends"
    assert np.array_equal(rec["hit"] != 0, depth > 0) and rec["hit"].sum() == hits
    assert np.array_equal(rec["trilinear"], info["trilinear"]) and np.array_equal(rec["r"].view(np.uint64), info["r"].view(np.uint64)), "r"
    assert np.array_equal(rec["depth"], bits(depth)) and np.array_equal(rec["xyz"], bits(xyz)) and np.array_equal(rec["normal"], bits(nrm))
    assert (rec["same_with_skip"] == 1).all(), "the skip moved a result"
    if shift == 0:
        assert 0 < info["trilinear"].sum() < hits                # both sources of r occur
