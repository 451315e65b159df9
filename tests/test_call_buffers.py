"""CPU suite: CallBuffers (cuda-slam_amd/csrc/call_buffers.hpp), the list in which a driver states each of its device buffers once -- reserve,
shape check, download -- checked on the host.  tests/call_buffers_selftest.cpp includes the header alone and supplies a malloc-backed, counting
allocator and a recording hipMemcpyAsync; it is built as a program of its own (no HIP runtime linked), plain and under the address and
undefined-behaviour sanitizers, and run."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

SOURCE = os.path.join(ROOT, "tests", "call_buffers_selftest.cpp")
ROCM = os.environ.get("ROCM", "/opt/rocm")


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]], ids=["plain", "sanitized"])
def test_call_buffers_state_each_buffer_once(tmp_path, flags):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "call_buffers_selftest")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROCM, "include")] + flags
                          + [SOURCE, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "call buffers selftest ok" in r.stdout, r.stdout + r.stderr
