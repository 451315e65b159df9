"""CPU suite: cuda-slam_amd/csrc/eval_block.hpp, the host arithmetic of mi_evaluate_registration behind its sums (the fitness, the inlier
RMSE, the 21 -> 36 expansion into the information matrix), checked on the host.  tests/eval_block_selftest.cpp includes the header alone; it
is built as a program of its own (no HIP runtime, nothing of HIP on the include path), plain and under the address and undefined-behaviour
sanitizers, and run."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

SOURCE = os.path.join(ROOT, "tests", "eval_block_selftest.cpp")


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]], ids=["plain", "sanitized"])
def test_eval_block_keeps_its_contract(tmp_path, flags):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "eval_block_selftest")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off"] + flags + [SOURCE, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "eval_block selftest ok" in r.stdout, r.stdout + r.stderr
