"""CPU suite: cuda-slam_amd/csrc/scan_context_bin.hpp, the arithmetic between a point and its bin of mi_scan_context, checked on the host.
tests/scan_context_bin_selftest.cpp includes the header alone; it is built as a program of its own (no HIP runtime, nothing of HIP on the
include path), plain and under the address and undefined-behaviour sanitizers, and run."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

SOURCE = os.path.join(ROOT, "tests", "scan_context_bin_selftest.cpp")


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]], ids=["plain", "sanitized"])
def test_scan_context_bins_keep_their_contract(tmp_path, flags):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "scan_context_bin_selftest")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off"] + flags + [SOURCE, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "scan_context_bin selftest ok" in r.stdout, r.stdout + r.stderr
