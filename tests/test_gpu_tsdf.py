"""GPU suite: mi_tsdf_integrate and mi_tsdf_extract against tests/tsdf_reference.py.  Coordinates, weights, row counts and order exactly;
values, points and normals bit for bit, without a tolerance anywhere: ray counts around a wave and a workgroup, S = 1, 6 and 16, rays on
the lattice's own planes and centres, rays shorter than the band, gates that drop everything; poses; input maps, the cap and the capacity
protocol; the extraction on fused scenes and on hand-made maps; the loop closed through mi_icp_plane_register; refusals and hygiene."""
import ctypes as C

import numpy as np
import pytest

import tsdf_reference as R
from test_tsdf_reference import ORIGIN, same_map, sphere

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def shell(seed, n, lo=1.0, hi=3.0):
    """n points at distances lo .. hi from the sensor, all around it"""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    return (d / np.linalg.norm(d, axis=1)[:, None] * rng.uniform(lo, hi, (n, 1))).astype(np.float32)


def pose(yaw, t, pitch=0.0):
    cy, sy, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    T = np.eye(4)
    T[:3, :3] = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1]]) @ np.array([[cp, 0, sp], [0, 1, 0], [-sp, 0, cp]])
    T[:3, 3] = t
    return T.astype(np.float32).astype(np.float64)


def corner_scan(seed, n, T):
    """n points on the three walls x = 0, y = 0, z = 0 of a room corner (0 .. 3 along each), in the frame of a sensor at pose T"""
    rng = np.random.default_rng(seed)
    uv = rng.uniform(0.05, 3.0, (n, 2))
    wall = rng.integers(0, 3, n)
    world = np.zeros((n, 3))
    for a in range(3):
        world[wall == a] = np.insert(uv[wall == a], a, 0.0, axis=1)
    return ((world - T[:3, 3]) @ T[:3, :3]).astype(np.float32)


CORNER_ORIGIN = np.array([0.03, 0.02, 0.01], np.float32)        # inside the scene: the walls lie at voxel coordinates around -1 and 0
CORNER_POSES = [pose(0.3, [1.5, 1.2, 1.0]), pose(-0.4, [1.0, 1.6, 1.3], 0.2), pose(1.1, [1.8, 0.9, 0.8], -0.1), pose(2.0, [1.2, 1.1, 1.6], 0.15),
                pose(0.7, [1.4, 1.4, 1.1], 0.05)]


def fuse(ctx, capi, scans, poses, origin, voxel, tau, map=None, **kw):
    return ctx.tsdf_integrate(scans, None if poses is None else np.array(poses), origin, capi.tsdf_params(voxel_size=voxel, truncation=tau, **kw), map=map)


def check(ctx, capi, scans, poses, origin, voxel, tau, map=None, **kw):
    got = fuse(ctx, capi, scans, poses, origin, voxel, tau, map=map, **kw)
    want = R.integrate(scans, poses, origin, voxel, tau, map=map, **kw)
    assert got[0].shape == want[0].shape and np.array_equal(got[0], want[0]), "coordinates, count or order"
    assert np.array_equal(bits(got[2]), bits(want[2])), "weights"
    assert np.array_equal(bits(got[1]), bits(want[1])), "values: %d of %d differ" % ((bits(got[1]) != bits(want[1])).sum(), len(want[1]))
    return got


def raw_integrate(ctx, capi, xyz, offsets, T, origin, params, m, capacity, K=None, fill=-7):
    xyz, offsets, origin = np.ascontiguousarray(xyz, np.float32), np.ascontiguousarray(offsets, np.int64), np.ascontiguousarray(origin, np.float32)
    T = None if T is None else np.ascontiguousarray(T, np.float32)
    room = max(int(capacity), 1)
    outs = (np.full((room, 3), fill, np.int32), np.full(room, fill, np.float32), np.full(room, fill, np.float32))
    nv = C.c_longlong(fill)
    m = m if m is not None else (None, None, None)
    nv_in = 0 if m[0] is None else len(m[0])
    rc = capi.tsdf_integrate_raw(ctx._h, xyz.ctypes.data, offsets.ctypes.data, len(offsets) - 1 if K is None else K, None if T is None else T.ctypes.data,
                                 origin.ctypes.data, C.addressof(params), *[None if a is None else a.ctypes.data for a in m], nv_in,
                                 *[a.ctypes.data if capacity else None for a in outs], int(capacity), C.addressof(nv))
    return rc, nv.value, outs, capi.lib().mi_last_error().decode()


def raw_extract(ctx, capi, m, origin, voxel, min_weight, capacity, want_normals=True, fill=-7.5):
    origin = np.ascontiguousarray(origin, np.float32)
    room = max(int(capacity), 1)
    xyz, nrm = np.full((room, 3), fill, np.float32), np.full((room, 3), fill, np.float32)
    n = C.c_longlong(-7)
    rc = capi.tsdf_extract_raw(ctx._h, m[0].ctypes.data, m[1].ctypes.data, m[2].ctypes.data, len(m[0]), origin.ctypes.data, float(voxel), float(min_weight),
                               xyz.ctypes.data if capacity else None, nrm.ctypes.data if capacity and want_normals else None, int(capacity), C.addressof(n))
    return rc, n.value, xyz, nrm, capi.lib().mi_last_error().decode()


# ---- 1. rays
def test_ray_counts(ctx, capi):
    # one ray, around a wave, several waves, several workgroups, one more than a workgroup's TSDF_BLOCK rays; S = 6
    for n in (1, 63, 64, 65, 257, 5000, capi.TSDF_BLOCK + 1):
        check(ctx, capi, [shell(n, n)], None, ORIGIN - 1, 0.1, 0.3)


@pytest.mark.parametrize("tau,S", [(0.05, 1), (0.3, 6), (0.8, 16)])
def test_half_steps(ctx, capi, tau, S):
    assert R.half_steps(0.1, tau) == S
    for n in (65, 5000):
        got = check(ctx, capi, [shell(100 + n, n)], None, ORIGIN - 1, 0.1, tau)
        assert len(got[0]) > n // 2


def test_rays_on_the_lattice_and_rays_shorter_than_the_band(ctx, capi):
    origin = np.zeros(3, np.float32)
    scans = [np.array([[4.5, 0, 0], [0, 4.5, 0], [0, 0, -2.5]], np.float32),       # along the axes through voxel centres, samples on lattice planes
             np.array([[2, 0, 0], [0, 3, 0], [2, 2, 0]], np.float32),               # lying in the lattice plane z = 1
             np.array([[0.25, 0, 0], [0.05, 0.05, 0.05], [0, -0.5, 0], [0, 0, 0]], np.float32)]      # shorter than the band; the last one has no length
    poses = [pose(0, [0, 0.5, 0.5]), pose(0, [0.5, 0.5, 1]), pose(0, [0.125, 0.125, 0.125])]
    poses[0][:3, 3] = [0.5, 0.5, 0.5]
    got = check(ctx, capi, scans, poses, origin, 1.0, 1.0)
    assert len(got[0]) > 0
    check(ctx, capi, scans, poses, origin, 0.25, 0.5)
    check(ctx, capi, scans[2:], poses[2:], np.full(3, -8, np.float32), 0.25, 2.0)


def test_gates_that_drop_every_ray(ctx, capi):
    pts = shell(7, 300)
    for kw in (dict(min_range=100.0), dict(max_range=0.5), dict(min_range=3.5, max_range=3.75)):
        got = check(ctx, capi, [pts], None, ORIGIN, 0.1, 0.3, **kw)
        assert len(got[0]) == 0
    stored = R.integrate([shell(8, 50)], None, ORIGIN, 0.1, 0.3)
    got = check(ctx, capi, [pts], None, ORIGIN, 0.1, 0.3, map=stored, min_range=100.0)
    assert same_map(got, stored)                                                    # *out_nv == nv_in, the map unchanged
    some = check(ctx, capi, [pts], None, ORIGIN, 0.1, 0.3, min_range=1.5, max_range=2.5)
    assert 0 < len(some[0]) < len(R.integrate([pts], None, ORIGIN, 0.1, 0.3)[0])


# ---- 2. poses
def test_poses(ctx, capi):
    scans = [corner_scan(20 + i, n, T) for i, (n, T) in enumerate(zip((700, 0, 1300), CORNER_POSES))]
    check(ctx, capi, scans[:1], None, CORNER_ORIGIN, 0.1, 0.3)                      # K = 1, no poses
    got = check(ctx, capi, scans, CORNER_POSES[:3], CORNER_ORIGIN, 0.1, 0.3)        # K = 3, an empty scan in the middle
    assert got[0].min() < 0 < got[0].max()                                          # a lattice with negative coordinates
    assert same_map(fuse(ctx, capi, scans, CORNER_POSES[:3], CORNER_ORIGIN, 0.1, 0.3), got)      # the same call twice
    ctx.voxel_downsample(shell(1, 3000), 0.2)                                       # other entry points use the context in between
    ctx.knn_search(None, shell(2, 500), 4)
    ctx.tsdf_extract(got, CORNER_ORIGIN, 0.1)
    assert same_map(fuse(ctx, capi, scans, CORNER_POSES[:3], CORNER_ORIGIN, 0.1, 0.3), got)
    times = ctx.tsdf_times()
    assert set(times) == set(capi.Context._TIMES["tsdf"]) and times["total"] > 0 and all(v >= 0 for v in times.values())


# ---- 3. input maps
def test_fusing_onto_a_map(ctx, capi):
    a, b = corner_scan(30, 900, CORNER_POSES[0]), corner_scan(31, 1100, CORNER_POSES[1])
    first = check(ctx, capi, [a], CORNER_POSES[:1], CORNER_ORIGIN, 0.1, 0.3)
    second = check(ctx, capi, [b], CORNER_POSES[1:2], CORNER_ORIGIN, 0.1, 0.3, map=first)
    assert len(second[0]) > len(first[0]) and second[2].max() > first[2].max()
    # a map disjoint from the rays passes through among the new rows
    far = (np.array([[400, 410, 420], [401, 410, 420], [-500, 0, 430]], np.int32), np.array([-0.0, 0.3333333, 1.0], np.float32), np.array([1e-30, 7.5, 3e38], np.float32))
    both = check(ctx, capi, [a], CORNER_POSES[:1], CORNER_ORIGIN, 0.1, 0.3, map=far)
    assert len(both[0]) == len(first[0]) + 3


def test_the_cap_binds(ctx, capi):
    scans = [shell(40, 400, 1.9, 2.1)] * 3
    once = check(ctx, capi, scans, None, ORIGIN, 0.1, 0.3, max_weight=2.0)
    assert once[2].max() == 2.0
    m = None
    for s in scans:
        m = check(ctx, capi, [s], None, ORIGIN, 0.1, 0.3, map=m, max_weight=2.0)
    assert (m[2] == 2.0).all() and np.array_equal(m[0], once[0])
    check(ctx, capi, scans[:1], None, ORIGIN, 0.1, 0.3, map=m, max_weight=0.5)     # a cap below the stored weight


def test_the_capacity_protocol(ctx, capi):
    pts = shell(50, 500)
    params = capi.tsdf_params(voxel_size=0.1, truncation=0.3)
    want = R.integrate([pts], None, ORIGIN, 0.1, 0.3)
    rc, nv, outs, _ = raw_integrate(ctx, capi, pts, [0, len(pts)], None, ORIGIN, params, None, 0)            # counts only
    assert rc == capi.MI_OK and nv == len(want[0])
    rc, nv, outs, _ = raw_integrate(ctx, capi, pts, [0, len(pts)], None, ORIGIN, params, None, len(want[0]) - 1)      # one row short
    assert rc == capi.MI_OK and nv == len(want[0])
    assert (outs[0] == -7).all() and (outs[1] == -7).all() and (outs[2] == -7).all()
    rc, nv, outs, _ = raw_integrate(ctx, capi, pts, [0, len(pts)], None, ORIGIN, params, None, len(want[0]) + 5)      # room to spare
    assert rc == capi.MI_OK and nv == len(want[0]) and same_map(tuple(o[:nv] for o in outs), want)
    assert (outs[0][nv:] == -7).all() and (outs[1][nv:] == -7).all() and (outs[2][nv:] == -7).all()


# ---- 4. extraction
def check_extract(ctx, m, origin, voxel, min_weight=1.0):
    xyz, nrm = ctx.tsdf_extract(m, origin, voxel, min_weight)
    want_xyz, want_nrm = R.extract(m, origin, voxel, min_weight)
    assert xyz.shape == want_xyz.shape, "count: %s against %s" % (xyz.shape, want_xyz.shape)
    assert same(xyz, want_xyz), "points: %d differ" % (bits(xyz) != bits(want_xyz)).any(axis=1).sum()
    assert same(nrm, want_nrm), "normals: %d differ" % (bits(nrm) != bits(want_nrm)).any(axis=1).sum()
    assert same(ctx.tsdf_extract(m, origin, voxel, min_weight, want_normals=False)[0], want_xyz)           # out_normals == NULL
    return xyz, nrm


def test_extraction_of_fused_scenes(ctx, capi):
    ball = check(ctx, capi, [sphere(2000)], None, ORIGIN, 0.1, 0.3)
    xyz, nrm = check_extract(ctx, ball, ORIGIN, 0.1)
    rad = np.linalg.norm(xyz.astype(np.float64), axis=1)
    assert len(xyz) > 500 and np.abs(rad - 2).max() <= 2 * 0.0154 * 0.1             # the twin's bar (test_tsdf_reference.py)
    scans = [corner_scan(60 + i, 1500, T) for i, T in enumerate(CORNER_POSES[:3])]
    room = check(ctx, capi, scans, CORNER_POSES[:3], CORNER_ORIGIN, 0.1, 0.3)
    xyz, nrm = check_extract(ctx, room, CORNER_ORIGIN, 0.1)
    assert len(xyz) > 1000
    few = check_extract(ctx, room, CORNER_ORIGIN, 0.1, min_weight=3.0)[0]
    assert 0 < len(few) < len(xyz)
    assert ctx.tsdf_extract(room, CORNER_ORIGIN, 0.1, min_weight=1e6)[0].shape == (0, 3)      # a min_weight that removes everything: *out_n == 0


def test_extraction_of_small_maps(ctx, capi):
    origin, w = np.zeros(3, np.float32), np.ones(2, np.float32)
    two = np.array([[5, 5, 5], [6, 5, 5]], np.int32)
    for values in ([0.5, -0.5], [0.0, 0.25], [0.0, 0.0], [1.0, -1.0], [0.5, 0.25], [-0.5, -0.0], [1.0, -0.125], [-1.0, 1.0]):
        check_extract(ctx, (two, np.array(values, np.float32), w), origin, 0.5)
    xyz, nrm = ctx.tsdf_extract((two, np.array([0.5, -0.5], np.float32), w), origin, 0.5)
    assert np.array_equal(xyz, [[3.0, 2.75, 2.75]]) and np.array_equal(nrm, [[-1.0, 0.0, 0.0]])
    # missing neighbours: a neighbour below min_weight, voxels apart, an L, a negative lattice, a 3 x 3 x 3 block with holes
    check_extract(ctx, (two, np.array([0.5, -0.5], np.float32), np.array([1.0, 0.5], np.float32)), origin, 0.5)
    check_extract(ctx, (np.array([[5, 5, 5], [7, 5, 5]], np.int32), np.array([0.5, -0.5], np.float32), w), origin, 0.5)
    ell = (np.array([[5, 5, 5], [6, 5, 5], [5, 6, 5]], np.int32), np.array([0.25, -0.75, -0.25], np.float32), np.ones(3, np.float32))
    assert len(check_extract(ctx, ell, origin, 0.5)[0]) == 2
    rng = np.random.default_rng(5)
    grid = np.stack(np.meshgrid(np.arange(-2, 3), np.arange(-2, 3), np.arange(-2, 3), indexing="ij"), axis=-1).reshape(-1, 3)[:, ::-1]
    grid = grid[rng.uniform(size=len(grid)) < 0.7].astype(np.int32)
    block = (grid, rng.choice([-1.0, -0.5, -0.0, 0.0, 0.25, 1.0], len(grid)).astype(np.float32), rng.choice([0.5, 1.0, 4.0], len(grid)).astype(np.float32))
    assert len(check_extract(ctx, block, np.array([0.3, -0.2, 0.1], np.float32), 0.25)[0]) > 10
    check_extract(ctx, block, np.array([0.3, -0.2, 0.1], np.float32), 0.25, min_weight=0.25)


def test_the_extraction_capacity_protocol(ctx, capi):
    m = R.integrate([sphere(600)], None, ORIGIN, 0.1, 0.3)
    want_xyz, want_nrm = R.extract(m, ORIGIN, 0.1)
    n = len(want_xyz)
    rc, found, xyz, nrm, _ = raw_extract(ctx, capi, m, ORIGIN, 0.1, 1.0, 0)
    assert rc == capi.MI_OK and found == n > 0
    rc, found, xyz, nrm, _ = raw_extract(ctx, capi, m, ORIGIN, 0.1, 1.0, n - 1)
    assert rc == capi.MI_OK and found == n and (xyz == -7.5).all() and (nrm == -7.5).all()
    rc, found, xyz, nrm, _ = raw_extract(ctx, capi, m, ORIGIN, 0.1, 1.0, n + 3)
    assert rc == capi.MI_OK and found == n and same(xyz[:n], want_xyz) and same(nrm[:n], want_nrm) and (xyz[n:] == -7.5).all() and (nrm[n:] == -7.5).all()
    rc, found, xyz, nrm, _ = raw_extract(ctx, capi, m, ORIGIN, 0.1, 1.0, n, want_normals=False)
    assert rc == capi.MI_OK and found == n and same(xyz, want_xyz) and (nrm == -7.5).all()
    rc, found, xyz, nrm, _ = raw_extract(ctx, capi, m, ORIGIN, 0.1, 1e6, n)
    assert rc == capi.MI_OK and found == 0 and (xyz == -7.5).all()


# ---- 5. the loop closed: scans -> poses -> map -> the next scan's registration target
def test_the_next_scan_registers_onto_the_extracted_surface(ctx, capi):
    scans = [corner_scan(70 + i, 4000, T) for i, T in enumerate(CORNER_POSES[:4])]
    room = check(ctx, capi, scans, CORNER_POSES[:4], CORNER_ORIGIN, 0.1, 0.3)
    tile, normals = check_extract(ctx, room, CORNER_ORIGIN, 0.1)
    ref_tile, ref_normals = R.extract(R.integrate(scans, CORNER_POSES[:4], CORNER_ORIGIN, 0.1, 0.3), CORNER_ORIGIN, 0.1)
    truth = CORNER_POSES[4]
    fifth = corner_scan(75, 3000, truth)
    start = pose(0.7 + 0.02, truth[:3, 3] + [0.05, -0.04, 0.03], 0.05 - 0.015)
    params = capi.plane_params(max_distance_squared=0.09, max_iterations=50)
    Rg, tg, itg, errg, whyg = ctx.icp_plane_register(fifth, tile, normals, params, init=start)
    Rr, tr, itr, errr, whyr = ctx.icp_plane_register(fifth, ref_tile, ref_normals, params, init=start)
    # the same bits in, the same bits out
    assert same(Rg, Rr) and same(tg, tr) and (itg, whyg) == (itr, whyr) and np.float32(errg).tobytes() == np.float32(errr).tobytes()
    # the surface lies within a fraction of a voxel of the walls (test_tsdf_reference.py), so the pose comes back to well within one voxel
    # (0.1) over a scene of 3 units: translation within 0.1, rotation within 0.1 / 3
    dt, dR = np.abs(tg - truth[:3, 3]).max(), np.abs(Rg - truth[:3, :3]).max()
    print("plane ICP onto the extracted surface: stop %d after %d iterations, |dt| %.4f, |dR| %.5f" % (whyg, itg, dt, dR))
    assert itg > 0 and dt <= 0.1 and dR <= 0.1 / 3


# ---- 6. refusals
def test_refusals(ctx, capi):
    pts = shell(80, 40)
    off = [0, 15, 40]
    good = capi.tsdf_params(voxel_size=0.1, truncation=0.3)
    T = np.tile(np.eye(4, dtype=np.float32).ravel(), (2, 1))
    m = R.integrate([shell(81, 20)], None, ORIGIN, 0.1, 0.3)
    m = tuple(np.ascontiguousarray(a) for a in m)

    def refused(word, xyz=pts, offsets=off, poses=T, origin=ORIGIN, params=good, map=None, capacity=4000, K=None, code=None):
        rc, nv, outs, msg = raw_integrate(ctx, capi, xyz, offsets, poses, origin, params, map, capacity, K=K)
        assert rc == (capi.MI_ERR_INVALID_ARG if code is None else code) and msg.startswith("mi_tsdf_integrate") and word in msg, (rc, msg)
        assert nv == -7 and (outs[0] == -7).all() and (outs[1] == -7).all() and (outs[2] == -7).all(), msg

    refused("K = 0", K=0)
    refused("scan_offsets[0]", offsets=[1, 15, 40])
    refused("descend at index 2", offsets=[0, 15, 14])
    refused("end at 0", offsets=[0, 0, 0])
    for value in (np.nan, np.inf, -2e18):
        bad = pts.copy()
        bad[33, 1] = value
        bad[35, 0] = value
        refused("scans_xyz point 33 ", xyz=bad)
    badT = T.copy()
    badT[1, 13] = np.inf
    refused("scan_T of scan 1 ", poses=badT)
    refused("origin3", origin=[0, np.nan, 0])
    for kw, word in ((dict(voxel_size=0.0), "voxel_size"), (dict(voxel_size=np.inf), "voxel_size"), (dict(truncation=0.04), "truncation"),
                     (dict(truncation=np.nan), "truncation"), (dict(min_range=-1.0), "min_range"), (dict(max_range=0.0), "max_range"),
                     (dict(min_range=2.0, max_range=2.0), "max_range"), (dict(max_weight=0.0), "max_weight"), (dict(max_weight=np.nan), "max_weight"),
                     (dict(truncation=0.86), "MI_TSDF_MAX_HALF_STEPS")):
        fields = dict(voxel_size=0.1, truncation=0.3)
        fields.update(kw)
        refused(word, params=capi.tsdf_params(**fields))
    refused("point 7 has a voxel coordinate outside", xyz=np.where(np.arange(40)[:, None] == 7, np.float32(3e5), pts), params=capi.tsdf_params(voxel_size=1e-4, truncation=1e-4))
    wide = pts.copy()
    wide[5] = [2000, 0, 0]
    refused("extent along axis 0", xyz=wide, params=capi.tsdf_params(voxel_size=1e-3, truncation=1e-3))
    swapped = (m[0].copy(), m[1], m[2])
    swapped[0][[3, 4]] = swapped[0][[4, 3]]
    refused("in_coord row 4 is not above row 3", map=swapped)
    twice = (m[0].copy(), m[1], m[2])
    twice[0][6] = twice[0][5]
    refused("in_coord row 6 ", map=twice)
    for value in (0.0, -1.0, np.inf, np.nan):
        w = m[2].copy()
        w[[2, 9]] = value
        refused("in_weight row 2 ", map=(m[0], m[1], w))
    for value in (1.5, -1.0000001, np.nan):
        d = m[1].copy()
        d[[8, 11]] = value
        refused("in_tsdf row 8 ", map=(m[0], d, m[2]))
    reach = (m[0].copy(), m[1], m[2])
    reach[0][-1] = [0, 0, 1 << 30]
    refused("in_coord row %d has a coordinate outside" % (len(m[0]) - 1), map=reach)
    reach[0][-1] = [0, 0, (1 << 30) - 1]
    refused("extent along axis 2", map=reach)
    refused("capacity = -1", capacity=-1)
    rc = capi.tsdf_integrate_raw(ctx._h, None, None, 1, None, None, None, None, None, None, 0, None, None, None, 0, None)
    assert rc == capi.MI_ERR_INVALID_ARG and capi.lib().mi_last_error().decode().startswith("mi_tsdf_integrate: null")
    big = np.array([0, 1 << 26], np.int64)                                          # 2^26 rays of 33 samples: 2^31 entries or more; no point is read
    rc, nv, outs, msg = raw_integrate(ctx, capi, pts, big, None, ORIGIN, capi.tsdf_params(voxel_size=0.1, truncation=0.8), None, 0)
    assert rc == capi.MI_ERR_INVALID_ARG and "2^31" in msg and nv == -7

    def refused_extract(word, map=m, origin=ORIGIN, voxel=0.1, min_weight=1.0, capacity=4000):
        rc, found, xyz, nrm, msg = raw_extract(ctx, capi, map, origin, voxel, min_weight, capacity)
        assert rc == capi.MI_ERR_INVALID_ARG and msg.startswith("mi_tsdf_extract") and word in msg, (rc, msg)
        assert found == -7 and (xyz == -7.5).all() and (nrm == -7.5).all(), msg

    refused_extract("coord row 4 is not above row 3", map=swapped)
    refused_extract("weight row 2 ", map=(m[0], m[1], np.where(np.isin(np.arange(len(m[2])), [2, 9]), np.float32(0), m[2])))
    refused_extract("tsdf row 8 ", map=(m[0], np.where(np.isin(np.arange(len(m[1])), [8, 11]), np.float32(np.nan), m[1]), m[2]))
    refused_extract("extent along axis 2", map=reach)
    refused_extract("voxel_size", voxel=0.0)
    refused_extract("min_weight", min_weight=0.0)
    refused_extract("min_weight", min_weight=np.nan)
    refused_extract("origin3", origin=[np.inf, 0, 0])
    refused_extract("capacity = -2", capacity=-2)
    # the context is as usable as before
    check(ctx, capi, [pts], None, ORIGIN, 0.1, 0.3)


def test_a_distributed_context_is_refused(capi):
    with capi.Context(0, 0, 1, exchange=lambda array, kind: None) as dist:      # one rank over the caller's transport: distributed all the same
        with pytest.raises(capi.MiSlamError, match="error %d" % capi.MI_ERR_STATE):
            fuse(dist, capi, [shell(1, 50)], None, ORIGIN, 0.1, 0.3)
        with pytest.raises(capi.MiSlamError, match="error %d" % capi.MI_ERR_STATE):
            dist.tsdf_extract(R.integrate([shell(1, 50)], None, ORIGIN, 0.1, 0.3), ORIGIN, 0.1)


# ---- 7. hygiene
def test_a_loaded_icp_problem_survives_and_nothing_leaks(ctx, capi, golden):
    z = golden.npz("synth2k_clouds.npz")
    icp = capi.icp_params(max_iterations=8)
    ctx.icp_load(z["before"], z["after"], icp)
    ctx.icp_run(8)
    R0, t0, it0, err0, why0 = ctx.icp_result()
    ctx.icp_load(z["before"], z["after"], icp)
    m = fuse(ctx, capi, [shell(90, 2000)], None, ORIGIN, 0.1, 0.3)
    ctx.tsdf_extract(m, ORIGIN, 0.1)
    ctx.icp_run(8)
    R1, t1, it1, err1, why1 = ctx.icp_result()
    assert it0 > 0 and (it1, why1) == (it0, why0)
    assert same(R1, R0) and same(t1, t0) and np.float32(err1).tobytes() == np.float32(err0).tobytes()

    # 20 calls of alternating sizes: the buffers grow once and no more
    clouds = [shell(91, 300), shell(92, 2000)]

    def alternate(i):
        got = fuse(ctx, capi, [clouds[i % 2]], None, ORIGIN, 0.1, 0.3)
        ctx.tsdf_extract(got, ORIGIN, 0.1, want_normals=bool(i % 3))

    alternate(0), alternate(1)
    ctx.synchronize()
    before = capi.selftest_live_buffers()
    for i in range(20):
        alternate(i)
    ctx.synchronize()
    assert capi.selftest_live_buffers() <= before
    assert same_map(fuse(ctx, capi, [shell(90, 2000)], None, ORIGIN, 0.1, 0.3), m)
