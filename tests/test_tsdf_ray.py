"""CPU suite: cuda-slam_amd/csrc/tsdf_ray.hpp, the arithmetic of mi_tsdf_integrate and mi_tsdf_extract between a posed point and its samples
and between two voxels and their crossing, checked on the host.  tests/tsdf_ray_selftest.cpp includes the header alone; it is built as a
program of its own (no HIP runtime, nothing of HIP on the include path), plain and under the address and undefined-behaviour sanitizers,
and run."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

SOURCE = os.path.join(ROOT, "tests", "tsdf_ray_selftest.cpp")


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]], ids=["plain", "sanitized"])
def test_tsdf_rays_keep_their_contract(tmp_path, flags):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "tsdf_ray_selftest")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off"] + flags + [SOURCE, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "tsdf_ray selftest ok" in r.stdout, r.stdout + r.stderr
