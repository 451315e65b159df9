"""GPU suite: mi_tsdf_mesh against tests/tsdf_mesh_reference.py, bit for bit on coordinates, normals and indices, without a tolerance
anywhere: every row of the triangle table, shared vertices on a noise lattice, a closed sphere, holes, a saturated step, a fused scan, the
shapes at which the kernels and the scan take another path, the capacity protocol in every branch, every refusal, and hygiene."""
import ctypes as C
import functools

import numpy as np
import pytest

import tsdf_mesh_reference as M
import tsdf_reference as R
from test_tsdf_mesh_reference import HOLES, ORIGIN, VOXEL

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def frozen(mp):
    out = tuple(np.ascontiguousarray(a) for a in mp)
    for a in out:
        a.setflags(write=False)
    return out


def rows_of(coord, values, weight=None):
    """a map of the listed voxels, in the map's order (cz, cy, cx)"""
    coord = np.asarray(coord, np.int64)
    order = np.lexsort((coord[:, 0], coord[:, 1], coord[:, 2]))
    weight = np.ones(len(coord), np.float32) if weight is None else np.asarray(weight, np.float32)
    return frozen((coord[order].astype(np.int32), np.asarray(values, np.float32)[order], weight[order]))


@functools.lru_cache(maxsize=None)
def scene(name):
    """(map, origin) of a named scene, built once and frozen"""
    if name == "noise":
        return frozen(M.noise_map(12, 1)), ORIGIN
    if name == "sphere":
        return frozen(M.sphere_map(12, 4.0)), ORIGIN
    if name == "holes":
        coord, tsdf, weight = M.sphere_map(12, 4.0)
        weight[HOLES] = 0.5
        return frozen((coord, tsdf, weight)), ORIGIN
    if name == "cases":
        # 256 blocks of 2 x 2 x 2 voxels, 16 x 16 of them three voxels apart: block c has its corners signed by case c
        rng = np.random.default_rng(76)
        coord, values = [], []
        for c in range(256):
            for k in range(8):
                coord.append(np.array([3 * (c % 16), 3 * (c // 16), 0]) + M.corner_offset(k))
                values.append(rng.uniform(0.1, 0.9) * (1 if c >> k & 1 else -1))
        return rows_of(coord, values), ORIGIN
    if name == "slab":
        # 41 x 40 x 2 = 3 280 rows: 13 workgroups of 256 rows and 4 tiles of the scan's 1 024 counts, the last of both part full
        z, y, x = np.meshgrid(np.arange(2), np.arange(40), np.arange(41), indexing="ij")
        coord = np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1)
        return rows_of(coord, np.random.default_rng(77).uniform(-0.9, 0.9, len(coord))), ORIGIN
    if name == "negative":
        coord, tsdf, weight = M.noise_map(7, 3)
        return frozen((coord - np.array([3, 40, 5], np.int32), tsdf, weight)), ORIGIN
    if name == "far":
        # voxel coordinates up to the last accepted ones, 2^30 - 1 and -2^30
        coord, tsdf, weight = M.noise_map(6, 4)
        return frozen((coord + np.array([2 ** 30 - 6, -2 ** 30, 2 ** 29], np.int32), tsdf, weight)), np.array([1e5, -2e5, 3.5], np.float32)
    if name == "wide":
        # two lattices 1 500 voxels apart along x and 1 100 along z: an extent above 1 024 on two axes
        a, b = M.noise_map(5, 5), M.sphere_map(8, 2.5)
        return rows_of(np.concatenate([a[0], b[0] + np.array([1500, 2, 1100], np.int32)]), np.concatenate([a[1], b[1]])), ORIGIN
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def reference(name, min_weight=1.0):
    mp, origin = scene(name)
    m = M.mesh(mp, origin, VOXEL, min_weight)
    for a in m:
        a.setflags(write=False)
    return m


def device(ctx, name, min_weight=1.0, normals=True):
    mp, origin = scene(name)
    return ctx.tsdf_mesh(mp, origin, VOXEL, min_weight, normals=normals)


def check(ctx, name, min_weight=1.0):
    want = reference(name, min_weight)
    xyz, normals, tri = device(ctx, name, min_weight)
    print("%s: %d vertices, %d triangles (reference %d, %d)" % (name, len(xyz), len(tri), len(want.xyz), len(want.tri)))
    assert xyz.shape == want.xyz.shape and tri.shape == want.tri.shape and tri.dtype == np.int32
    assert np.array_equal(tri, want.tri), "indices: %d of %d triangles differ" % ((tri != want.tri).any(axis=1).sum(), len(tri))
    assert np.array_equal(bits(xyz), bits(want.xyz)), "coordinates"
    assert np.array_equal(bits(normals), bits(want.normals)), "normals"
    return want, xyz, normals, tri


def raw(ctx, capi, mp, origin, vcap, tcap, voxel=VOXEL, min_weight=1.0, normals=True, nv=None, null=()):
    """one mi_tsdf_mesh with arrays of max(capacity, 1) rows filled with -7: (rc, nvert, ntri, xyz, normals, tri, message)"""
    origin = np.ascontiguousarray(origin, np.float32)
    xyz, nrm = np.full((max(vcap, 1), 3), -7.5, np.float32), np.full((max(vcap, 1), 3), -7.5, np.float32)
    tri = np.full((max(tcap, 1), 3), -7, np.int32)
    nvert, ntri = C.c_longlong(-7), C.c_longlong(-7)
    ptr = lambda key, a: None if key in null or a is None else a.ctypes.data
    rc = capi.tsdf_mesh_raw(ctx._h, ptr("coord", mp[0]), ptr("tsdf", mp[1]), ptr("weight", mp[2]), len(mp[1]) if nv is None else nv,
                            ptr("origin", origin), float(voxel), float(min_weight), ptr("xyz", xyz), ptr("normals", nrm if normals else None), int(vcap),
                            None if "nvert" in null else C.addressof(nvert), ptr("tri", tri), int(tcap), None if "ntri" in null else C.addressof(ntri))
    return rc, nvert.value, ntri.value, xyz, nrm, tri, capi.lib().mi_last_error().decode()


# ---- 1. the table
def test_every_case(ctx):
    want, _, _, tri = check(ctx, "cases")
    mp, _ = scene("cases")
    heads = np.nonzero((mp[0] % 3 == 0).all(axis=1))[0]                # the blocks' first corners, in row order
    case_of_block = (mp[0][heads, 0] // 3 + 16 * (mp[0][heads, 1] // 3)).astype(np.int64)
    assert np.array_equal(np.nonzero(want.meshed)[0], heads) and np.array_equal(want.case[heads], case_of_block)      # one meshed cube per block
    assert len(tri) == 820 and np.array_equal(np.bincount(want.tri_cube, minlength=len(mp[1]))[heads], [len(M.TABLE[c]) for c in case_of_block])


# ---- 2. shared vertices, closed surfaces, holes
def test_shared_vertices_on_the_noise_lattice(ctx):
    want, xyz, _, tri = check(ctx, "noise")
    mp, _ = scene("noise")
    edges, open_edges = M.check_shared_edges(mp, 1.0, want, tri=tri)
    assert edges == 3 * len(tri) and 0 < open_edges < edges // 10
    assert len(np.unique(tri)) == len(xyz)


def test_a_closed_surface(ctx):
    want, xyz, normals, tri = check(ctx, "sphere")
    mp, _ = scene("sphere")
    a, b = M.directed_edges(tri)
    undirected, count = np.unique(np.minimum(a, b) * len(xyz) + np.maximum(a, b), return_counts=True)
    assert (count == 2).all() and len(xyz) - len(undirected) + len(tri) == 2
    assert M.check_shared_edges(mp, 1.0, want, tri=tri)[1] == 0
    g = M.geometric_normals(xyz, tri)
    assert ((g[:, None, :] * normals[tri].astype(np.float64)).sum(axis=2) > 0).all()
    assert (M.check_positive_side(mp, want, xyz=xyz, tri=tri) > 0).all()


def test_holes(ctx):
    want, xyz, normals, tri = check(ctx, "holes")
    whole = reference("sphere")
    mp, origin = scene("holes")
    assert 0 < len(tri) < len(whole.tri) and not want.meshed[HOLES].any()
    for h in HOLES:                                                    # the cubes that held the voxel are gone
        near = (np.abs(mp[0].astype(np.int64) - mp[0][h]).max(axis=1) <= 1) & (mp[0] <= mp[0][h]).all(axis=1)
        assert not want.meshed[near].any() and not np.isin(np.nonzero(near)[0], want.tri_cube).any()
    points, point_normals = ctx.tsdf_extract(mp, origin, VOXEL)
    assert len(xyz) < len(points) and len(np.unique(tri)) == len(xyz)  # a strict subset, every vertex referenced ...
    at = np.searchsorted(M.crossing_keys(mp[0].astype(np.int64), mp[1], mp[2] >= 1, R._Table(mp[0].astype(np.int64), mp[2] >= 1)), want.vert_key)
    assert (np.diff(at) > 0).all() and np.array_equal(bits(points[at]), bits(xyz)) and np.array_equal(bits(point_normals[at]), bits(normals))       # ... of mi_tsdf_extract's rows
    # below min_weight is the same as absent: a min_weight under the holes' 0.5 brings the whole sphere back
    back = ctx.tsdf_mesh(mp, origin, VOXEL, 0.25)
    assert np.array_equal(back[2], whole.tri) and np.array_equal(bits(back[0]), bits(whole.xyz)) and np.array_equal(bits(back[1]), bits(whole.normals))


def test_a_saturated_edge(ctx):
    z, y, x = np.meshgrid(np.arange(3), np.arange(3), np.arange(4), indexing="ij")
    coord = np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1).astype(np.int32)
    weight = np.ones(len(coord), np.float32)
    step = np.where(coord[:, 0] < 2, 1.0, -1.0).astype(np.float32)     # +1 beside -1: no crossing, and the cubes over the step are not meshed
    xyz, normals, tri = ctx.tsdf_mesh((coord, step, weight), ORIGIN, VOXEL)
    assert xyz.shape == (0, 3) and normals.shape == (0, 3) and tri.shape == (0, 3)
    # one saturated edge among crossings: the cubes round it vanish, the others stay
    mixed = np.where(coord[:, 0] < 2, 1.0, -0.5).astype(np.float32)
    mixed[(coord == [2, 1, 1]).all(axis=1)] = -1.0
    mp = (coord, mixed, weight)
    want = M.mesh(mp, ORIGIN, VOXEL)
    xyz, normals, tri = ctx.tsdf_mesh(mp, ORIGIN, VOXEL)
    assert not want.meshed[(coord[:, 0] == 1)].any() and len(want.tri) == 0 and len(tri) == 0 and len(xyz) == 0
    assert len(ctx.tsdf_extract(mp, ORIGIN, VOXEL)[0]) == 8            # (the other eight crossings are still mi_tsdf_extract's)
    wall = np.where(coord[:, 0] < 2, 1.0, -0.5).astype(np.float32)
    want = M.mesh((coord, wall, weight), ORIGIN, VOXEL)
    xyz, normals, tri = ctx.tsdf_mesh((coord, wall, weight), ORIGIN, VOXEL)
    assert len(tri) == 8 and np.array_equal(tri, want.tri) and np.array_equal(bits(xyz), bits(want.xyz)) and np.array_equal(bits(normals), bits(want.normals))


# ---- 3. through the pipeline
def test_a_fused_scan(ctx, capi):
    rng = np.random.default_rng(78)
    d = rng.normal(size=(6000, 3))
    ball = (0.8 * d / np.linalg.norm(d, axis=1)[:, None]).astype(np.float32)
    lattice = np.full(3, -1.5, np.float32)
    mp = ctx.tsdf_integrate([ball], None, lattice, capi.tsdf_params(voxel_size=0.1, truncation=0.3))
    want = M.mesh(mp, lattice, 0.1)
    xyz, normals, tri = ctx.tsdf_mesh(mp, lattice, 0.1)
    print("fused sphere: %d voxels, %d vertices, %d triangles" % (len(mp[1]), len(xyz), len(tri)))
    assert len(tri) > 1000 and np.array_equal(tri, want.tri) and np.array_equal(bits(xyz), bits(want.xyz)) and np.array_equal(bits(normals), bits(want.normals))
    radii = np.linalg.norm(xyz.astype(np.float64), axis=1)
    assert np.abs(radii - 0.8).max() <= 0.02                           # (mi_tsdf_extract's own points: within a fifth of a voxel of the sphere)
    g = M.geometric_normals(xyz, tri)
    centroid = xyz.astype(np.float64)[tri].mean(axis=1)
    assert ((g * centroid).sum(axis=1) < 0).mean() > 0.99              # wound towards the sensor at the centre


# ---- 4. shapes
@pytest.mark.parametrize("name", ["slab", "negative", "far", "wide"])
def test_shape_limits(ctx, name):
    want, xyz, _, tri = check(ctx, name)
    mp, _ = scene(name)
    assert len(tri) > 100 and len(np.unique(tri)) == len(xyz)
    if name == "slab":
        assert len(mp[1]) > 3 * 1024 and len(mp[1]) % 256 != 0 and len(tri) > 1024 and len(xyz) > 1024
    if name == "far":
        assert mp[0].max() == 2 ** 30 - 1 and mp[0].min() == -2 ** 30
    if name == "wide":
        extent = mp[0].max(axis=0).astype(np.int64) - mp[0].min(axis=0) + 1
        assert extent[0] > 1024 and extent[2] > 1024


# ---- 5. the capacity protocol
def test_the_capacity_protocol(ctx, capi):
    mp, origin = scene("sphere")
    want = reference("sphere")
    nv, nt = len(want.xyz), len(want.tri)
    untouched = lambda xyz, nrm, tri: (xyz == -7.5).all() and (nrm == -7.5).all() and (tri == -7).all()
    rc, nvert, ntri, xyz, nrm, tri, msg = raw(ctx, capi, mp, origin, 0, 0, null=("xyz", "normals", "tri"))     # counts only
    assert (rc, nvert, ntri) == (capi.MI_OK, nv, nt), msg
    for vcap, tcap in ((nv - 1, nt), (nv, nt - 1), (0, nt), (nv, 0), (1, 1)):                                  # either capacity short
        rc, nvert, ntri, xyz, nrm, tri, msg = raw(ctx, capi, mp, origin, vcap, tcap)
        assert (rc, nvert, ntri) == (capi.MI_OK, nv, nt) and untouched(xyz, nrm, tri), (vcap, tcap, msg)
    for vcap, tcap in ((nv, nt), (nv + 5, nt + 3)):
        rc, nvert, ntri, xyz, nrm, tri, msg = raw(ctx, capi, mp, origin, vcap, tcap)
        assert (rc, nvert, ntri) == (capi.MI_OK, nv, nt), msg
        assert np.array_equal(tri[:nt], want.tri) and np.array_equal(bits(xyz[:nv]), bits(want.xyz)) and np.array_equal(bits(nrm[:nv]), bits(want.normals))
        assert untouched(xyz[nv:], nrm[nv:], tri[nt:])
    rc, nvert, ntri, xyz, nrm, tri, msg = raw(ctx, capi, mp, origin, nv, nt, normals=False)                     # NULL normals
    assert (rc, nvert, ntri) == (capi.MI_OK, nv, nt) and np.array_equal(tri, want.tri) and np.array_equal(bits(xyz), bits(want.xyz)) and (nrm == -7.5).all()
    got = device(ctx, "sphere", normals=False)
    assert got[1] is None and np.array_equal(got[2], want.tri)
    # nothing to mesh: two zero counts, nothing written, whatever the capacities
    empty = (np.zeros((0, 3), np.int32), np.zeros(0, np.float32), np.zeros(0, np.float32))
    for m, null in ((empty, ("coord", "tsdf", "weight")), ((mp[0], np.abs(mp[1]), mp[2]), ()), ((mp[0], mp[1], mp[2] * np.float32(0.5)), ())):
        rc, nvert, ntri, xyz, nrm, tri, msg = raw(ctx, capi, m, origin, 10, 10, null=null)
        assert (rc, nvert, ntri) == (capi.MI_OK, 0, 0) and untouched(xyz, nrm, tri), msg
    xyz, nrm, tri = ctx.tsdf_mesh(None, origin, VOXEL)
    assert xyz.shape == (0, 3) and nrm.shape == (0, 3) and tri.shape == (0, 3)


# ---- 6. refusals
def test_refusals(ctx, capi):
    mp, origin = scene("sphere")
    want = reference("sphere")
    nv, nt = len(want.xyz), len(want.tri)

    def refused(word, m=mp, o=origin, vcap=nv, tcap=nt, code=None, **kw):
        rc, nvert, ntri, xyz, nrm, tri, msg = raw(ctx, capi, m, o, vcap, tcap, **kw)
        assert rc == (capi.MI_ERR_INVALID_ARG if code is None else code) and msg.startswith("mi_tsdf_mesh") and word in msg, (rc, msg)
        assert nvert == -7 and ntri == -7 and (xyz == -7.5).all() and (nrm == -7.5).all() and (tri == -7).all(), msg

    refused("null origin3", null=("origin",))
    refused("out_nvert", null=("nvert",))
    refused("out_ntri", null=("ntri",))
    refused("nv = -1", nv=-1)
    for key in ("coord", "tsdf", "weight"):
        refused("null coord, tsdf or weight", null=(key,))
    for voxel in (0.0, -0.1, np.inf, np.nan):
        refused("voxel_size", voxel=voxel)
    for w in (0.0, -1.0, np.nan):
        refused("min_weight", min_weight=w)
    refused("origin3 not finite", o=[0, np.inf, 0])
    refused("vertex_capacity = -1", vcap=-1)
    refused("tri_capacity = -2", tcap=-2)
    refused("null out_xyz", null=("xyz",))
    refused("null out_tri", null=("tri",))
    refused("null out_xyz", null=("xyz",), tcap=0)
    refused("null out_tri", null=("tri",), vcap=0)
    coord, tsdf, weight = (a.copy() for a in mp)
    swapped = coord.copy()
    swapped[[3, 4]] = swapped[[4, 3]]
    refused("coord row 4 is not above row 3", m=(swapped, tsdf, weight))
    twice = coord.copy()
    twice[8] = twice[7]
    refused("coord row 8 is not above row 7", m=(twice, tsdf, weight))
    out = coord.copy()
    out[-1, 2] = 2 ** 30
    refused("coord row %d has a coordinate outside" % (len(out) - 1), m=(out, tsdf, weight))
    wide = coord.copy()
    wide[-1, 2] = 2 ** 20 + 5
    refused("extent along axis 2", m=(wide, tsdf, weight))
    for value in (np.nan, 1.5, -np.inf):
        bad = tsdf.copy()
        bad[11] = value
        refused("tsdf row 11", m=(coord, bad, weight))
    for value in (0.0, -1.0, np.inf, np.nan):
        bad = weight.copy()
        bad[13] = value
        refused("weight row 13", m=(coord, tsdf, bad))
    # and the call still works
    rc, nvert, ntri, xyz, nrm, tri, msg = raw(ctx, capi, mp, origin, nv, nt)
    assert (rc, nvert, ntri) == (capi.MI_OK, nv, nt) and np.array_equal(tri, want.tri)


def test_a_distributed_context_is_refused(capi):
    mp, origin = scene("sphere")
    with capi.Context(0, 0, 1, exchange=lambda array, kind: None) as dist:      # one rank over the caller's transport: distributed all the same
        rc, nvert, ntri, xyz, nrm, tri, msg = raw(dist, capi, mp, origin, 400, 700)
        assert rc == capi.MI_ERR_STATE and msg.startswith("mi_tsdf_mesh") and nvert == -7 and ntri == -7 and (tri == -7).all() and (xyz == -7.5).all(), (rc, msg)


# ---- 7. hygiene
def test_two_calls_give_the_same_bits_and_a_loaded_icp_problem_survives(ctx, capi, golden):
    z = golden.npz("synth2k_clouds.npz")
    icp = capi.icp_params(max_iterations=8)
    ctx.icp_load(z["before"], z["after"], icp)
    ctx.icp_run(8)
    R0, t0, it0, err0, why0 = ctx.icp_result()
    ctx.icp_load(z["before"], z["after"], icp)
    first = device(ctx, "noise")
    device(ctx, "slab")                                                # another size in between: the buffers grow and are reused
    ctx.tsdf_extract(scene("sphere")[0], ORIGIN, VOXEL)
    second = device(ctx, "noise")
    ctx.icp_run(8)
    R1, t1, it1, err1, why1 = ctx.icp_result()
    assert it0 > 0 and (it1, why1) == (it0, why0)
    assert np.array_equal(bits(R1), bits(R0)) and np.array_equal(bits(t1), bits(t0)) and np.float32(err1).tobytes() == np.float32(err0).tobytes()
    assert np.array_equal(first[2], second[2]) and np.array_equal(bits(first[0]), bits(second[0])) and np.array_equal(bits(first[1]), bits(second[1]))
    times = ctx.tsdf_times()
    assert len(times) == 8 and times["total"] > 0
    ctx.synchronize()
    before = capi.selftest_live_buffers()
    for i in range(10):
        device(ctx, ("noise", "slab")[i % 2], normals=bool(i % 3))
    ctx.synchronize()
    assert capi.selftest_live_buffers() <= before
