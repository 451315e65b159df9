"""GPU suite: mi_tsdf_raycast against tests/tsdf_raycast_reference.py.  Depth, point and normal bits and the hit count are the reference's,
without a tolerance anywhere, with empty-space skipping and with every sample visited: ray counts around a wave and a workgroup; rays
along the axes, in lattice planes, from inside the band, from behind and out of unobserved space on hand-made slabs; pinhole and spherical
views of the corner room, also with the scene far from zero, where fp32 positions are as coarse as the voxels; the empty map, the optional
outputs, refusals, hygiene, the loop closed through mi_icp_plane_register, and K71's table with a probe chain past its last slot."""
import ctypes as C
import functools

import numpy as np
import pytest

import ndt_scale_cases as S
import tsdf_raycast_reference as RC
import tsdf_reference as R
from test_gpu_tsdf import CORNER_ORIGIN, CORNER_POSES, check_extract, corner_scan, pose, same, shell
from test_tsdf_reference import ORIGIN

pytestmark = pytest.mark.gpu

FILL = -7.5


def raw(ctx, capi, m, origin, params, T, dirs, n=None, want=(True, True, True), nv=None):
    """(rc, depth, xyz, normals, hits, message) of one call through the C interface, the outputs pre-filled with FILL / -7"""
    dirs = np.ascontiguousarray(dirs, np.float32)
    n = len(dirs) if n is None else n
    origin = None if origin is None else np.ascontiguousarray(origin, np.float32)
    T = None if T is None else np.ascontiguousarray(T, np.float32)
    room = max(len(dirs), 1)
    depth, xyz, nrm, hits = np.full(room, FILL, np.float32), np.full((room, 3), FILL, np.float32), np.full((room, 3), FILL, np.float32), C.c_longlong(-7)
    m = (None, None, None) if m is None else tuple(np.ascontiguousarray(a) for a in m)
    nv = (0 if m[0] is None else len(m[0])) if nv is None else nv
    rc = capi.tsdf_raycast_raw(ctx._h, *[None if a is None else a.ctypes.data for a in m], nv, None if origin is None else origin.ctypes.data,
                               None if params is None else C.addressof(params), None if T is None else T.ctypes.data, dirs.ctypes.data, n, depth.ctypes.data,
                               xyz.ctypes.data if want[0] else None, nrm.ctypes.data if want[1] else None, C.addressof(hits) if want[2] else None)
    return rc, depth, xyz, nrm, hits.value, capi.lib().mi_last_error().decode()


def check(ctx, capi, m, origin, voxel, max_range, T, dirs, **kw):
    """both marches against the reference: the full rows with skipping, the compacted ones with every sample visited"""
    want = RC.raycast(m, origin, voxel, max_range, T, dirs, **kw)
    depth, xyz, nrm = ctx.tsdf_raycast(m, origin, capi.tsdf_raycast_params(voxel_size=voxel, max_range=max_range, **kw), T, dirs)
    assert same(depth, want[0]), "depths: %d of %d differ" % ((depth.view(np.uint32) != want[0].view(np.uint32)).sum(), len(depth))
    assert same(xyz, want[1]), "points: %d differ" % (xyz.view(np.uint32) != want[1].view(np.uint32)).any(axis=1).sum()
    assert same(nrm, want[2]), "normals: %d differ" % (nrm.view(np.uint32) != want[2].view(np.uint32)).any(axis=1).sum()
    index = np.nonzero(want[0] > 0)[0]
    assert len(index) == want[3]
    d1, x1, n1, i1 = ctx.tsdf_raycast(m, origin, capi.tsdf_raycast_params(voxel_size=voxel, max_range=max_range, visit_every_sample=1, **kw), T, dirs, compact=True)
    assert np.array_equal(i1, index) and same(d1, want[0][index]) and same(x1, want[1][index]) and same(n1, want[2][index]), "every sample visited"
    return want


@functools.lru_cache(maxsize=None)
def shell_map():
    return R.integrate([shell(5000, 5000)], None, ORIGIN - 1, 0.1, 0.3)


@functools.lru_cache(maxsize=None)
def corner_room(shift=0.0):
    """four scans of the corner fused by the reference; the scene, the poses and the lattice moved by shift (1, -1, 1/2)"""
    move = np.array([shift, -shift, shift / 2])
    poses = []
    for T in CORNER_POSES:
        T = T.copy()
        T[:3, 3] = (T[:3, 3] + move).astype(np.float32)
        poses.append(T)
    origin = (CORNER_ORIGIN.astype(np.float64) + move).astype(np.float32)
    scans = [corner_scan(70 + i, 4000, T) for i, T in enumerate(CORNER_POSES[:4])]
    return R.integrate(scans, poses[:4], origin, 0.1, 0.3), origin, poses


def mounted(dirs, forward):
    """camera directions (z ahead, x right, y down) in the frame of a sensor that carries the camera looking along `forward`"""
    f = np.asarray(forward, np.float64) / np.linalg.norm(forward)
    right = np.cross(f, [0, 0, 1.0])
    right /= np.linalg.norm(right)
    down = np.cross(f, right)
    return (dirs.astype(np.float64) @ np.stack([right, down, f])).astype(np.float32)


def views(capi):
    return {"pinhole": mounted(capi.pinhole_directions(80, 60, 40.0, 40.0, 39.5, 29.5), [1.0, -0.6, -0.3]),
            "spherical": capi.spherical_directions(16, 256, -0.6, 0.6)}


# ---- 1. ray counts
def test_ray_counts(ctx, capi):
    # one ray, around a wave, several waves, several workgroups, one more than a workgroup; K = floor(4 / 0.05f) + 1 = 80 (the float 0.1 is a
    # little above 0.1)
    assert RC.steps(0.1, 0, 4) == 80
    total = 0
    for n in (1, 63, 64, 65, 257, 5000, capi.TSDF_BLOCK + 1):
        dirs = np.random.default_rng(n).normal(size=(n, 3)).astype(np.float32)
        total += check(ctx, capi, shell_map(), ORIGIN - 1, 0.1, 4.0, None, dirs)[3]
    assert total > 500


# ---- 2. grazing and axis rays
@pytest.mark.parametrize("voxel", [1.0, 0.25])
def test_axis_and_grazing_rays_on_a_slab(ctx, capi, voxel):
    v = voxel
    m = RC.slab(5.25 * v, tau=4.0 * v, voxel=v)
    origin = np.zeros(3, np.float32)
    axes = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [0, 0, 0], [-0.0, 0, 0], [3, 0, 0], [1, 1, 0], [1, 0, 1], [2, -1, 0.5]], np.float32)

    def at(x, y, z):
        T = np.eye(4)
        T[:3, 3] = np.array([x, y, z]) * v
        return T

    hits = 0
    hits += check(ctx, capi, m, origin, v, 9.0 * v, at(0.5, 4.5, 4.5), axes)[3]          # through voxel centres: samples on lattice planes and centres
    hits += check(ctx, capi, m, origin, v, 9.0 * v, at(0.5, 4.0, 4.0), axes)[3]          # in the lattice planes y = 4 and z = 4
    hits += check(ctx, capi, m, origin, v, 9.0 * v, at(0.0, 0.0, 0.0), axes)[3]          # along the map's edge
    assert hits >= 6
    assert check(ctx, capi, m, origin, v, 9.0 * v, at(3.5, 4.3, 3.7), axes)[3] >= 1       # starting inside the band, on the positive side
    assert check(ctx, capi, m, origin, v, 9.0 * v, at(6.5, 4.3, 3.7), axes)[3] == 0       # inside the negative side: every ray misses
    assert check(ctx, capi, m, origin, v, 14.0 * v, at(-5.0, 4.3, 3.7), axes)[3] >= 1     # out of unobserved space in front of the band
    assert check(ctx, capi, m, origin, v, 9.0 * v, at(9.5, 4.3, 3.7), axes)[3] == 0       # out of unobserved space behind it
    assert check(ctx, capi, m, origin, v, 9.0 * v, at(0.25, 4.3, 3.7), axes, min_range=3.0 * v)[3] >= 1      # min_range inside the band
    assert check(ctx, capi, m, origin, v, 9.0 * v, at(0.25, 4.3, 3.7), axes, min_range=5.5 * v)[3] == 0      # ... and behind the surface
    assert RC.steps(v, 0, 0.25 * v) == 1
    assert check(ctx, capi, m, origin, v, 0.25 * v, at(4.9, 4.3, 3.7), axes)[3] == 0      # K = 1: a single sample cannot hit
    assert RC.steps(v, 0, 0.5 * v) == 2
    assert check(ctx, capi, m, origin, v, 0.5 * v, at(4.9, 4.3, 3.7), axes[:1])[3] == 1   # K = 2: the shortest march that can
    assert check(ctx, capi, m, origin, v, 9.0 * v, at(0.25, 4.3, 3.7), axes, min_weight=1.5)[3] == 0         # no voxel is observed


# ---- 3. the corner room; 4. the skip moves no bit, also far from zero
@pytest.mark.parametrize("shift", [0.0, 3e4, 2e6])
def test_views_of_the_corner_room(ctx, capi, shift):
    m, origin, poses = corner_room(shift)
    tilted = pose(2.4, [1.1, 1.7, 1.4], -0.5)
    tilted[:3, 3] = (tilted[:3, 3] + np.array([shift, -shift, shift / 2])).astype(np.float32)
    for T in (poses[4], tilted):
        for name, dirs in views(capi).items():
            for min_weight in (1.0, 2.0):
                want = check(ctx, capi, m, origin, 0.1, 5.0, T, dirs, min_weight=min_weight)
                if shift != 2e6:         # (there fp32 positions are 0.25 apart: the map is a coarse one, and what it shows the reference decides)
                    assert 0 < want[3] < len(dirs), "%s, min_weight %g: %d hits of %d" % (name, min_weight, want[3], len(dirs))


# ---- 5. the empty map, optional outputs
def test_the_empty_map_and_the_optional_outputs(ctx, capi):
    dirs = shell(3, 300)
    for m in (None, (np.zeros((0, 3), np.int32), np.zeros(0, np.float32), np.zeros(0, np.float32))):
        depth, xyz, nrm = ctx.tsdf_raycast(m, ORIGIN, capi.tsdf_raycast_params(voxel_size=0.1, max_range=4.0), None, dirs)
        assert not depth.any() and not xyz.any() and not nrm.any()
    params = capi.tsdf_raycast_params(voxel_size=0.1, max_range=4.0)
    rc, depth, xyz, nrm, hits, msg = raw(ctx, capi, None, ORIGIN, params, None, dirs)
    assert rc == capi.MI_OK and hits == 0 and not depth.any() and not xyz.any() and not nrm.any(), msg
    m = shell_map()
    want = RC.raycast(m, ORIGIN - 1, 0.1, 4.0, None, dirs)
    assert want[3] > 0
    for absent in range(3):
        asked = tuple(i != absent for i in range(3))
        rc, depth, xyz, nrm, hits, msg = raw(ctx, capi, m, ORIGIN - 1, params, None, dirs, want=asked)
        assert rc == capi.MI_OK and same(depth, want[0]), msg
        assert same(xyz, want[1]) if asked[0] else (xyz == FILL).all()
        assert same(nrm, want[2]) if asked[1] else (nrm == FILL).all()
        assert hits == (want[3] if asked[2] else -7)
    rc, depth, xyz, nrm, hits, msg = raw(ctx, capi, m, ORIGIN - 1, params, None, dirs, want=(False, False, False))
    assert rc == capi.MI_OK and same(depth, want[0])
    # fewer rays than the arrays hold: the rows behind n stay as they were
    rc, depth, xyz, nrm, hits, msg = raw(ctx, capi, m, ORIGIN - 1, params, None, dirs, n=100)
    assert rc == capi.MI_OK and same(depth[:100], want[0][:100]) and (depth[100:] == FILL).all() and (xyz[100:] == FILL).all() and hits == (want[0][:100] > 0).sum()
    times = ctx.tsdf_times()
    assert times["total"] > 0 and all(v >= 0 for v in times.values())


# ---- 6. refusals
def test_refusals(ctx, capi):
    m = tuple(np.ascontiguousarray(a) for a in shell_map())
    dirs = shell(4, 40)
    good = capi.tsdf_raycast_params(voxel_size=0.1, max_range=4.0)
    eye = np.eye(4, dtype=np.float32).ravel()

    def refused(word, map=m, origin=ORIGIN - 1, params=good, T=eye, d=dirs, n=None, nv=None, code=None):
        rc, depth, xyz, nrm, hits, msg = raw(ctx, capi, map, origin, params, T, d, n=n, nv=nv)
        assert rc == (capi.MI_ERR_INVALID_ARG if code is None else code) and msg.startswith("mi_tsdf_raycast") and word in msg, (rc, msg)
        assert hits == -7 and (depth == FILL).all() and (xyz == FILL).all() and (nrm == FILL).all(), msg

    refused("null", origin=None)
    refused("null", params=None)
    refused("null coord, tsdf or weight", map=None, nv=5)
    rc = capi.tsdf_raycast_raw(ctx._h, None, None, None, 0, ORIGIN.ctypes.data, C.addressof(good), None, None, 3, None, None, None, None)
    assert rc == capi.MI_ERR_INVALID_ARG and capi.lib().mi_last_error().decode().startswith("mi_tsdf_raycast: null")
    refused("n = 0", n=0)
    refused("n = -3", n=-3)
    refused("nv = -1", nv=-1)
    for kw, word in ((dict(voxel_size=0.0), "voxel_size"), (dict(voxel_size=np.inf), "voxel_size"), (dict(voxel_size=np.nan), "voxel_size"),
                     (dict(min_weight=0.0), "min_weight"), (dict(min_weight=np.nan), "min_weight"), (dict(min_range=-1.0), "min_range"),
                     (dict(min_range=np.inf), "min_range"), (dict(max_range=0.0), "max_range"), (dict(min_range=2.0, max_range=2.0), "max_range"),
                     (dict(max_range=np.inf), "max_range"), (dict(max_range=np.nan), "max_range"), (dict(visit_every_sample=2), "visit_every_sample"),
                     (dict(voxel_size=1e-3, max_range=32.8), "MI_TSDF_RAYCAST_MAX_STEPS")):
        fields = dict(voxel_size=0.1, max_range=4.0)
        fields.update(kw)
        refused(word, params=capi.tsdf_raycast_params(**fields))
    assert RC.steps(1e-3, 0, 32.7) <= 65536 < RC.steps(1e-3, 0, 32.8)
    badT = eye.copy()
    badT[13] = np.inf
    refused("T has a non-finite entry (entry 13)", T=badT)
    refused("origin3", origin=[0, np.nan, 0])
    for value in (np.nan, np.inf, -2e18):
        bad = dirs.copy()
        bad[33, 1] = value
        bad[35, 0] = value
        refused("dirs_xyz ray 33 ", d=bad)
    swapped = (m[0].copy(), m[1], m[2])
    swapped[0][[3, 4]] = swapped[0][[4, 3]]
    refused("coord row 4 is not above row 3", map=swapped)
    refused("weight row 2 ", map=(m[0], m[1], np.where(np.isin(np.arange(len(m[2])), [2, 9]), np.float32(0), m[2])))
    refused("tsdf row 8 ", map=(m[0], np.where(np.isin(np.arange(len(m[1])), [8, 11]), np.float32(np.nan), m[1]), m[2]))
    reach = (m[0].copy(), m[1], m[2])
    reach[0][-1] = [0, 0, 1 << 30]
    refused("coord row %d has a coordinate outside" % (len(m[0]) - 1), map=reach)
    reach[0][-1] = [0, 0, (1 << 30) - 1]
    refused("extent along axis 2", map=reach)
    # the context is as usable as before
    check(ctx, capi, m, ORIGIN - 1, 0.1, 4.0, None, dirs)


def test_a_distributed_context_is_refused(capi):
    with capi.Context(0, 0, 1, exchange=lambda array, kind: None) as dist:      # one rank over the caller's transport: distributed all the same
        with pytest.raises(capi.MiSlamError, match="error %d" % capi.MI_ERR_STATE):
            dist.tsdf_raycast(shell_map(), ORIGIN - 1, capi.tsdf_raycast_params(voxel_size=0.1, max_range=4.0), None, shell(1, 50))


# ---- 7. hygiene
def test_a_loaded_icp_problem_survives_and_nothing_leaks(ctx, capi, golden):
    z = golden.npz("synth2k_clouds.npz")
    icp = capi.icp_params(max_iterations=8)
    ctx.icp_load(z["before"], z["after"], icp)
    ctx.icp_run(8)
    R0, t0, it0, err0, why0 = ctx.icp_result()
    ctx.icp_load(z["before"], z["after"], icp)
    params = capi.tsdf_raycast_params(voxel_size=0.1, max_range=4.0)
    first = ctx.tsdf_raycast(shell_map(), ORIGIN - 1, params, None, shell(5, 2000))
    ctx.icp_run(8)
    R1, t1, it1, err1, why1 = ctx.icp_result()
    assert it0 > 0 and (it1, why1) == (it0, why0)
    assert same(R1, R0) and same(t1, t0) and np.float32(err1).tobytes() == np.float32(err0).tobytes()

    # 20 calls of alternating sizes and marches, other entry points in between: the buffers grow once and no more, and the bits stay
    small = (shell_map()[0][:4000], shell_map()[1][:4000], shell_map()[2][:4000])
    plain = capi.tsdf_raycast_params(voxel_size=0.1, max_range=4.0, visit_every_sample=1)

    def alternate(i):
        ctx.tsdf_raycast(small if i % 2 else shell_map(), ORIGIN - 1, plain if i % 3 == 0 else params, None, shell(6 + i % 2, 300 if i % 2 else 2000))

    def others():
        ctx.voxel_downsample(shell(1, 3000), 0.2)
        ctx.tsdf_extract(shell_map(), ORIGIN - 1, 0.1)

    alternate(0), alternate(1), others()
    ctx.synchronize()
    before = capi.selftest_live_buffers()
    for i in range(20):
        alternate(i)
        if i % 7 == 0:
            others()
    ctx.synchronize()
    assert capi.selftest_live_buffers() <= before
    again = ctx.tsdf_raycast(shell_map(), ORIGIN - 1, params, None, shell(5, 2000))
    assert all(same(a, b) for a, b in zip(again, first))


# ---- 8. the loop closed: integrate -> raycast from the last pose -> mi_icp_plane_register with init -> integrate
def test_the_next_scan_registers_onto_the_raycast_surface(ctx, capi):
    m, origin, poses = corner_room(0.0)
    truth = CORNER_POSES[4]
    fifth = corner_scan(75, 3000, truth)
    start = pose(0.7 + 0.02, truth[:3, 3] + [0.05, -0.04, 0.03], 0.05 - 0.015)
    dirs = capi.spherical_directions(32, 512, -1.2, 1.2)
    cast = capi.tsdf_raycast_params(voxel_size=0.1, max_range=5.0)
    depth, tile, normals, index = ctx.tsdf_raycast(m, origin, cast, start, dirs, compact=True)
    want = RC.raycast(m, origin, 0.1, 5.0, start, dirs)
    ref_index = np.nonzero(want[0] > 0)[0]
    assert np.array_equal(index, ref_index) and len(index) > 3000 and same(tile, want[1][ref_index]) and same(normals, want[2][ref_index])
    params = capi.plane_params(max_distance_squared=0.09, max_iterations=50)
    Rg, tg, itg, errg, whyg = ctx.icp_plane_register(fifth, tile, normals, params, init=start)
    Rr, tr, itr, errr, whyr = ctx.icp_plane_register(fifth, want[1][ref_index], want[2][ref_index], params, init=start)
    # the same bits in, the same bits out
    assert same(Rg, Rr) and same(tg, tr) and (itg, whyg) == (itr, whyr) and np.float32(errg).tobytes() == np.float32(errr).tobytes()
    # the bounds of test_the_next_scan_registers_onto_the_extracted_surface: translation within one voxel (0.1), rotation within 0.1 / 3
    dt, dR = np.abs(tg - truth[:3, 3]).max(), np.abs(Rg - truth[:3, :3]).max()
    print("plane ICP onto the raycast surface: %d points, stop %d after %d iterations, |dt| %.4f, |dR| %.5f" % (len(index), whyg, itg, dt, dR))
    assert itg > 0 and dt <= 0.1 and dR <= 0.1 / 3
    # and the scan goes into the map at the pose found
    found = np.eye(4)
    found[:3, :3], found[:3, 3] = Rg, tg
    grown = ctx.tsdf_integrate([fifth], np.array([found]), origin, capi.tsdf_params(voxel_size=0.1, truncation=0.3), map=m)
    assert len(grown[0]) >= len(m[0]) and grown[2].max() > m[2].max()


# ---- 9. the table at its limit: tests/ndt_scale_cases.py's wrap map as a TSDF map, every row observed, so that K71's keys, capacity and
# home slots are the NDT case's and a probe chain goes past the last slot and on from slot 0
def test_a_map_whose_probe_chain_passes_the_last_slot(ctx, capi):
    vox = S.wrap_map()[0]
    coord = vox["coord"]
    coord = np.ascontiguousarray(coord[np.lexsort((coord[:, 0], coord[:, 1], coord[:, 2]))], np.int32)      # ascending by (cz, cy, cx)
    nv = len(coord)
    assert np.array_equal(coord, vox["coord"])                   # (so table_build's rows are this map's rows)
    assert S.table_build(vox, np.arange(nv))[1] >= 1 and S.table_build(vox, np.arange(nv)[::-1])[1] >= 1
    # values of either sign by the parity of the cell, so that every pair of listed neighbours has a crossing; every weight >= min_weight = 1
    rng = np.random.default_rng(293)
    tsdf = (rng.uniform(0.05, 1, nv) * np.where(coord.sum(axis=1) % 2 == 0, 1, -1)).astype(np.float32)
    m = (coord, tsdf, rng.uniform(1, 3, nv).astype(np.float32))
    origin, voxel = vox["origin"], float(vox["voxel"])
    xyz, _ = check_extract(ctx, m, origin, voxel)
    assert len(xyz) >= 30
    # 350 rays from inside the box: five towards every crossing, a little apart, and 100 anywhere
    T = np.eye(4, dtype=np.float32)
    T[:3, 3] = (origin.astype(np.float64) + (coord.min(axis=0) + 20.3) * voxel).astype(np.float32)
    aim = np.repeat(xyz.astype(np.float64) - T[:3, 3], 5, axis=0)
    dirs = np.concatenate([aim * (1 + 0.01 * rng.normal(size=aim.shape)), rng.normal(size=(100, 3))]).astype(np.float32)
    assert 20 <= check(ctx, capi, m, origin, voxel, 30.0, T, dirs)[3] < len(dirs)
