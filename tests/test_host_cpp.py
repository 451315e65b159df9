"""CPU suite: the C++ host side (cuda-slam_amd/host -> cuda-slam_amd/mi-slam): configuration reader quirks and the
clouds-from-configuration stage.  No GPU call is made (MISLAM_DUMP_ONLY stops the program before the registration)."""
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, noise_corpus, write_noise_meshes

EXE = os.path.join(ROOT, "cuda-slam_amd", "mi-slam")

BASE = {"before-path": "a.obj", "after-path": "a.obj", "method": "icp", "translation": [1.0, 1.0, 1.0],
        "rotation": [0.36, 0.47, -0.8, -0.8, 0.6, 0, 0.48, 0.64, 0.6]}


def run(cfg, tmp_path, *extra, dump=False):
    if not os.path.exists(EXE):
        pytest.skip("mi-slam not built (run __graft_entry__.build())")
    p = tmp_path / "cfg.json"
    p.write_text(json.dumps(cfg) if isinstance(cfg, dict) else cfg)
    args = [EXE, str(p), "--prepare", "host"] + list(extra)      # the device input stage is the GPU suite's (test_gpu_host_cpp.py)
    if dump:
        args += ["--dump-clouds", str(tmp_path / "clouds.bin")]
    env = dict(os.environ, MISLAM_DUMP_ONLY="1")
    return subprocess.run(args, capture_output=True, text=True, env=env, cwd=str(tmp_path), timeout=120)


def write_obj(path, verts, faces):
    with open(path, "w") as f:
        for v in verts:
            f.write("v %r %r %r\n" % tuple(float(x) for x in v))
        for fc in faces:
            f.write("f " + " ".join(str(i) for i in fc) + "\n")


def read_dump(path):
    n, m = np.fromfile(path, dtype=np.int32, count=2)
    d = np.fromfile(path, dtype=np.float32, offset=8)
    return d[:3 * n].reshape(n, 3), d[3 * n:].reshape(m, 3)


def test_parser_defaults_and_quirks(tmp_path):
    write_obj(tmp_path / "a.obj", [(0, 0, 0), (1, 0, 0), (0, 1, 0)], [(1, 2, 3)])
    r = run(BASE, tmp_path, dump=True)
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout
    assert "Approximation type: hybrid" in out            # configparser.cpp:217
    assert "const scale: 0" in out                        # parsed default false (configparser.cpp:240), not the struct's true
    assert "Max distance squared: 1000.0" in out and "Convergence epsilon: 0.001" in out
    cfg = dict(BASE, **{"approximation-type": "banana", "cpd-const-scale": True, "max-distance-squared": 400})
    out = run(cfg, tmp_path, dump=True).stdout
    assert "Approximation type: hybrid" in out and "const scale: 1" in out and "Max distance squared: 400.0" in out


def test_parser_rejects_like_the_reference(tmp_path):
    write_obj(tmp_path / "a.obj", [(0, 0, 0), (1, 0, 0), (0, 1, 0)], [(1, 2, 3)])
    no_transform = {k: v for k, v in BASE.items() if k not in ("translation", "rotation")}
    r = run(no_transform, tmp_path)
    assert r.returncode != 0 and "transformation or transformation parameters have to be provided" in r.stdout and "Aborting" in r.stdout
    # the parser reads "rotation-range", not the schema's "angle-range" (configparser.cpp:170 vs config/schema.json:42)
    assert run(dict(no_transform, **{"translation-range": 1.0, "angle-range": 0.2}), tmp_path).returncode != 0
    assert run(dict(no_transform, **{"translation-range": 1.0, "rotation-range": 0.2, "random-seed": 3}), tmp_path, dump=True).returncode == 0
    assert "not supported" in run(dict(BASE, method="ransac"), tmp_path).stdout
    assert "Wrong translation or rotation size" in run(dict(BASE, rotation=[1, 0, 0]), tmp_path).stdout
    assert run("{ this is not json", tmp_path).returncode != 0


def test_obj_face_corner_expansion_and_transform(tmp_path):
    # 4 vertices, one triangle + one quad: 3 + 4 = 7 points -- one per face corner AS WRITTEN, duplicates kept: the reference's loader copies
    # mesh->mVertices (loader.cpp:58-66), and assimp's triangulation only re-indexes the quad's four vertices (bird.obj: 8 752 quads = the
    # 35 008 points of testset.cpp:25-26; round 5: quads used to be fan-triangulated into 6 points here)
    verts = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)]
    write_obj(tmp_path / "a.obj", verts, [(1, 2, 3), (1, 2, 3, 4)])
    r = run(dict(BASE, **{"random-seed": 5}), tmp_path, dump=True)
    assert r.returncode == 0
    before, after = read_dump(tmp_path / "clouds.bin")
    assert before.shape == (7, 3) and after.shape == (7, 3)
    v = np.array(verts, np.float32)
    expect = np.concatenate([v[[0, 1, 2]], v[[0, 1, 2, 3]]])
    assert sorted(map(tuple, before)) == sorted(map(tuple, expect))
    R = np.array(BASE["rotation"], np.float32).reshape(3, 3)
    want = sorted(map(tuple, np.round(expect @ R.T + 1.0, 5)))
    assert np.allclose(sorted(map(tuple, np.round(after, 5))), want, atol=2e-5)


def test_negative_resize_returns_the_whole_cloud(tmp_path):
    # GetSubcloud compares `int subcloudSize >= cloud.size()` (common.cpp:27): the int is converted to size_t, so a negative
    # "cloud-*-resize" counts as huge and the cloud comes back whole, no permutation drawn; an in-range value subsamples
    verts = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)]
    write_obj(tmp_path / "a.obj", verts, [(1, 2, 3), (1, 2, 3, 4)])
    whole = run(dict(BASE, **{"random-seed": 5}), tmp_path, dump=True)
    b0, a0 = read_dump(tmp_path / "clouds.bin")
    r = run(dict(BASE, **{"random-seed": 5, "cloud-before-resize": -3, "cloud-after-resize": -1}), tmp_path, dump=True)
    assert whole.returncode == 0 and r.returncode == 0
    b1, a1 = read_dump(tmp_path / "clouds.bin")
    assert np.array_equal(b0, b1) and np.array_equal(a0, a1)
    r = run(dict(BASE, **{"random-seed": 5, "cloud-before-resize": 4}), tmp_path, dump=True)
    assert r.returncode == 0 and read_dump(tmp_path / "clouds.bin")[0].shape == (4, 3)


def test_bunny_input_stage_reproduces_the_golden_clouds(tmp_path, golden):
    # config/default.json + random-seed 666: same OBJ expansion, normalisation, shuffles and transform as the clouds the
    # reference's own preprocessing produced (tests/golden/bunny_clouds.npz) -- bit for bit.  The reference's data/bunny.obj is
    # rebuilt from the fixture (tests/golden/noise_meshes.npz: its vertex table and face corners, every fp32 value exact)
    _, meshes = noise_corpus(golden)
    write_noise_meshes({"bunny.obj": meshes["bunny.obj"]}, str(tmp_path))
    bunny = str(tmp_path / "data" / "bunny.obj")
    cfg = dict(BASE, **{"before-path": bunny, "after-path": bunny, "cloud-spread": 10.0, "random-seed": 666,
                        "max-distance-squared": 400, "max-iterations": 50, "policy": "parallel"})
    r = run(cfg, tmp_path, dump=True)
    assert r.returncode == 0
    before, after = read_dump(tmp_path / "clouds.bin")
    z = golden.npz("bunny_clouds.npz")
    assert np.array_equal(before, z["before"]) and np.array_equal(after, z["after"])
