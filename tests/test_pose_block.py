"""CPU suite: cuda-slam_amd/csrc/pose_block.hpp, the host arithmetic of the pose loop behind mi_icp_plane_register, mi_icp_gicp_register and
mi_ndt_register (the state block at a start pose, the check of a caller's transform, out_T and the error from a block, the batch rule), checked
on the host.  tests/pose_block_selftest.cpp includes the header alone; it is built as a program of its own (no HIP runtime, nothing of HIP
on the include path), plain and under the address and undefined-behaviour sanitizers, and run."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

SOURCE = os.path.join(ROOT, "tests", "pose_block_selftest.cpp")


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]], ids=["plain", "sanitized"])
def test_pose_block_keeps_its_contract(tmp_path, flags):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "pose_block_selftest")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off"] + flags + [SOURCE, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "pose_block selftest ok" in r.stdout, r.stdout + r.stderr
