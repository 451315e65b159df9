"""CPU suite: cuda-slam_amd/csrc/voxel_table.hpp, the voxel hash table of the NDT map, the TSDF map and the ray cast's skip blocks, checked on
the host.  tests/voxel_table_selftest.cpp includes the header alone; it is built as a program of its own (no HIP runtime, nothing of HIP on
the include path), plain and under the address and undefined-behaviour sanitizers, and run: once on its own facts, and once over the
1 000 voxels of tests/ndt_scale_cases.py's wrap map, where every row's key, hash and slot -- for two orders of insertion, with a probe chain
that goes past the last slot -- and the look-up of every cell of the listed box are compared with the numpy restatement there."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import ndt_scale_cases as S
from conftest import ROOT

SOURCE = os.path.join(ROOT, "tests", "voxel_table_selftest.cpp")


@pytest.fixture(scope="module", params=[[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]], ids=["plain", "sanitized"])
def selftest(request, tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("voxel_table") / "voxel_table_selftest")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off"] + request.param + [SOURCE, "-o", exe])
    return exe


def test_the_table_keeps_its_contract(selftest):
    r = subprocess.run([selftest], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "voxel_table selftest ok" in r.stdout, r.stdout + r.stderr


def test_the_header_builds_the_wrap_map_as_the_restatement_does(selftest, tmp_path):
    vox = S.wrap_map()[0]
    coord = vox["coord"].astype(np.int64)
    nv = len(coord)
    orders = [np.arange(nv), np.arange(nv)[::-1]]
    # the condition of this test: in either order a probe chain goes past the last slot and on from slot 0
    expected = [S.table_build(vox, order) for order in orders]
    assert nv == S.WRAP_NV and all(wrapped >= 1 for _, wrapped in expected)

    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as fh:
        fh.write(np.array([nv, len(orders)], "<i4").tobytes())
        fh.write(np.ascontiguousarray(coord, "<i4").tobytes())
        fh.write(np.ascontiguousarray(orders, "<i4").tobytes())
    r = subprocess.run([selftest, src, dst], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = open(dst, "rb").read()

    lo, side = coord.min(axis=0), S.WRAP_SIDE
    assert np.array_equal(lo, S.WRAP_BASE) and np.array_equal(coord.max(axis=0) - lo + 1, [side] * 3)
    slots, cells = np.frombuffer(raw, "<u8", 2)
    assert slots == S.table_capacity(nv) and cells == side ** 3
    keys, hashes = np.frombuffer(raw, "<u8", nv, offset=16), np.frombuffer(raw, "<u8", nv, offset=16 + 8 * nv)
    assert np.array_equal(keys, S.table_keys(coord)) and np.array_equal(hashes, S.table_hash(S.table_keys(coord)))

    # the row of every cell of the box, x fastest: the listed ones their row, every other one -1
    rel = coord - lo
    row_of = np.full(side ** 3, -1, np.int32)
    row_of[(rel[:, 2] * side + rel[:, 1]) * side + rel[:, 0]] = np.arange(nv)
    assert (row_of >= 0).sum() == nv
    per_order = np.dtype([("slot", "<i8", nv), ("found", "<i4", side ** 3)])
    got = np.frombuffer(raw, per_order, len(orders), offset=16 + 16 * nv)
    assert len(raw) == 16 + 16 * nv + len(orders) * per_order.itemsize
    for (slot_of, _), g in zip(expected, got):
        assert np.array_equal(g["slot"], slot_of)
        assert np.array_equal(g["found"], row_of)
    assert not np.array_equal(got[0]["slot"], got[1]["slot"])       # the order of arrival moves rows, and no look-up with them
