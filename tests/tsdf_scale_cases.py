"""The cases of tests/test_gpu_tsdf_scale.py and what they share: the scenes at which mi_tsdf_integrate, mi_tsdf_extract and mi_tsdf_raycast
leave the one small scene of tests/test_gpu_tsdf.py -- maps wider than 1024 voxels along chosen axes (the driver's 20-bit sort, frames above
1024), the extents 1024, 1025 and 2^20 made exact by stored rows, lattices whose occupied coordinates lie beyond +-2^29, a thousand scans
with empty ones at the start, the end and in runs, more rays than 256 tiles of the offsets scan, runs of thousands of samples in one voxel,
and stored weights at which W + C rounds.  tests/test_tsdf_scale_cases.py holds every case to its name with tests/tsdf_reference.py alone.

A case is a dict: scans (a list of [n, 3] float32 clouds in their sensors' frames), poses (a list of 4 x 4 matrices or None), origin,
voxel, tau, map (a triple to fuse onto, or None) and kw (further parameters of R.integrate and capi.tsdf_params).  Every case is cached,
seeded, and left unchanged by its users.  No tolerance is introduced here."""
import functools
import time

import numpy as np

import tsdf_reference as R
from test_gpu_tsdf import pose, shell

VOXEL, TAU = 0.1, 0.3
SORT_EXTENT = 1 << 10                # tsdf_api.hip: up to here along an axis the sort of that axis takes one 10-bit pass, above it two
MAX_EXTENT = 1 << 20                 # VOXEL_MAX_EXTENT (csrc/voxel_table.hpp)
LIMIT = 1 << 30                      # voxel coordinates lie in [-2^30, 2^30)
SCAN_TILE = 1024                     # RADIUS_SCAN_TILE (csrc/kernels.h): counts per tile of the offsets scan
SCAN_LANES = 256                     # lanes of the one workgroup that scans the tile sums
GAP = 115.0                          # between the poses of a wide case, along every wide axis: 1150 voxels
WIDE_AXES = ("x", "y", "z", "xz", "xyz")
NEAR_ORIGIN = np.array([-3.05, -3.02, -3.01], np.float32)


def frozen(a):
    a.setflags(write=False)
    return a


def frozen_map(m):
    return tuple(frozen(np.ascontiguousarray(a)) for a in m)


def case(scans, poses, origin, voxel=VOXEL, tau=TAU, map=None, **kw):
    return dict(scans=[frozen(np.ascontiguousarray(s, np.float32)) for s in scans], poses=None if poses is None else [frozen(np.array(T)) for T in poses],
                origin=frozen(np.asarray(origin, np.float32).copy()), voxel=voxel, tau=tau, map=None if map is None else frozen_map(map), kw=kw)


REFERENCE_SECONDS = {}               # by the cache key of reference(): what tests/test_tsdf_scale_cases.py prints


def integrate(c, scans=None, poses="own", map="own", **kw):
    """the reference's map of a case (or of some of its scans, under other poses, onto another map, with other parameters)"""
    args = dict(c["kw"])
    args.update(kw)
    return R.integrate(c["scans"] if scans is None else scans, c["poses"] if isinstance(poses, str) else poses, c["origin"], c["voxel"], c["tau"],
                       map=c["map"] if isinstance(map, str) else map, **args)


@functools.lru_cache(maxsize=None)
def reference(name, *args):
    """the reference's map of the case CASES[name](*args), computed once and frozen"""
    c = CASES[name](*args)
    t0 = time.perf_counter()
    m = frozen_map(integrate(c))
    REFERENCE_SECONDS[(name,) + args] = time.perf_counter() - t0
    return m


def extents(coord):
    coord = np.asarray(coord, np.int64)
    return tuple(int(v) for v in coord.max(axis=0) - coord.min(axis=0) + 1)


def longest_run(c, **kw):
    """the most samples any one voxel receives in a case"""
    coord = R.samples(c["scans"], c["poses"], c["origin"], c["voxel"], c["tau"], **kw)[0]
    return int(np.unique(coord, axis=0, return_counts=True)[1].max()) if len(coord) else 0


# ---- 1. wide axes
def ten_bit_order(coord):
    """the rows' order if every axis were sorted by the low 10 bits of its key alone (coordinate minus the axis minimum)"""
    rel = np.asarray(coord, np.int64) - np.asarray(coord, np.int64).min(axis=0)
    low = rel & (SORT_EXTENT - 1)
    return np.lexsort((low[:, 0], low[:, 1], low[:, 2]))


def wide_poses(axes):
    """three poses 0, GAP and 310 units along every axis named in `axes`, a little turned.  The third shell lies 3100 voxels from the
    first: 28 modulo 1024, so that a sort by the low 10 bits of the keys shuffles the two"""
    step = np.array([1.0 if a in axes else 0.0 for a in "xyz"])
    return [pose(0.3 * i, np.array([0.2, 0.1, -0.3]) + at * step, 0.1 * i) for i, at in enumerate((0.0, GAP, 310.0))]


@functools.lru_cache(maxsize=None)
def wide(axes):
    """three shells of 300 rays, radius 1 to 3, their sensors GAP and more apart along the axes named: above 1024 voxels there, under 100
    elsewhere"""
    return case([shell(300 + 10 * WIDE_AXES.index(axes) + i, 300) for i in range(3)], wide_poses(axes), NEAR_ORIGIN)


@functools.lru_cache(maxsize=None)
def edge_scan(extent):
    """(scan, pose, its own map): one shell of 200 rays over the middle of a range of `extent` voxels along x"""
    lo = 0 if extent <= 2048 else -(extent // 2)
    mid = (lo + extent // 2 + 0.5) * VOXEL + float(NEAR_ORIGIN[0])
    scan, T = shell(330 + extent % 7, 200), pose(0.4, [mid, 0.1, -0.3])
    return scan, T, lo, R.integrate([scan], [T], NEAR_ORIGIN, VOXEL, TAU)


@functools.lru_cache(maxsize=None)
def edge(extent):
    """one shell of 200 rays whose samples lie strictly between two stored rows `extent` - 1 voxels apart along x (1024: the last extent of
    the 10-bit sort; 1025: the first of the 20-bit one; 2^20: the last one accepted).  The stored rows lie in a line (cy, cz) that holds a
    voxel of the shell, so the three are neighbours in the map's order; their values and weights pass through, no sample reaches them"""
    scan, T, lo, own = edge_scan(extent)
    cy, cz = (int(v) for v in own[0][len(own[0]) // 2, 1:])
    stored = (np.array([[lo, cy, cz], [lo + extent - 1, cy, cz]], np.int32), np.array([0.25, -0.5], np.float32), np.array([2.0, 7.5], np.float32))
    return case([scan], [T], NEAR_ORIGIN, map=stored)


# ---- 2. far from zero
FAR = 1.05e8                         # |origin|: coordinates around 1.05e9 at voxel 0.1, between 2^29 and 2^30; fp32 positions are 8 apart there


def block_map(centre, values_seed):
    """a 5 x 5 x 5 block of voxels around `centre` with values of either sign by the parity of the cell (every pair of neighbours crosses)"""
    rng = np.random.default_rng(values_seed)
    g = np.stack(np.meshgrid(np.arange(-2, 3), np.arange(-2, 3), np.arange(-2, 3), indexing="ij"), axis=-1).reshape(-1, 3)[:, ::-1]
    coord = (g + np.asarray(centre, np.int64)).astype(np.int32)                # ascending by (cz, cy, cx)
    tsdf = (rng.uniform(0.05, 1, len(coord)) * np.where(g.sum(axis=1) % 2 == 0, 1, -1)).astype(np.float32)
    return coord, tsdf, rng.uniform(1, 3, len(coord)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def far(sign):
    """Two shells of 400 rays, radius 1 to 40, and one of 1500 rays, radius 1 to 3, on a lattice whose origin lies FAR from them: 'plus'
    (every coordinate around +1.05e9), 'minus' (-1.05e9), 'mixed' (+, -, near zero).  The fp32 difference p - origin is a multiple of 8 out
    there, 80 voxels: the samples collapse into few voxels, and the small shell's 1500 rays into the eight around its sensor at the most,
    so the runs are long.  A stored block around the first sensor's voxel goes in with them, so that the
    extraction and the ray cast of the fused map have neighbours to find at these coordinates."""
    origin = {"plus": [-FAR, -FAR, -FAR], "minus": [FAR, FAR, FAR], "mixed": [-FAR, FAR, 0.0]}[sign]
    poses = [pose(0.2, [0.5, -0.25, 0.75]), pose(-0.7, [9.0, 14.0, -11.0], 0.3), pose(1.3, [0.5, -0.25, 0.75], -0.2)]
    centre = R.voxel_of(np.array([0.5, -0.25, 0.75], np.float32), np.array(origin, np.float32), VOXEL)
    return case([shell(350, 400, 1.0, 40.0), shell(351, 400, 1.0, 40.0), shell(352, 1500)], poses, origin, map=block_map(centre, 353))


@functools.lru_cache(maxsize=None)
def far_poses():
    """the shells of a small scene seen from poses translated 1e5 units, the lattice's origin near zero: fp32 positions are 1 / 128 apart"""
    move = np.array([1e5, -1e5, 5e4])
    poses = [pose(0.2, move + [0.5, -0.25, 0.75]), pose(-0.7, move + [1.0, 0.5, 0.25], 0.3)]
    return case([shell(360 + i, 1500) for i in range(2)], poses, NEAR_ORIGIN)


# ---- 3. many scans
MANY_SCANS = 1000
EMPTY_SCANS = ((0, 3), (200, 1), (400, 2), (600, 17), (997, 3))       # (first scan, length) of every run of empty scans


@functools.lru_cache(maxsize=None)
def scan_lengths():
    n = np.random.default_rng(370).integers(1, 4, MANY_SCANS)
    for first, length in EMPTY_SCANS:
        n[first:first + length] = 0
    return frozen(n)


@functools.lru_cache(maxsize=None)
def many_scans(posed=True):
    """A thousand scans of 1 to 3 rays, but for the empty ones of EMPTY_SCANS, along a circle of radius 20: successive poses lie 0.15
    apart, more than a voxel, so a ray moved by its neighbour's pose lands in other voxels.  posed=False: the same offsets, scan_T = NULL."""
    n = scan_lengths()
    pts = shell(371, int(n.sum()))
    cuts = np.concatenate([[0], np.cumsum(n)])
    theta = 0.0075 * np.arange(MANY_SCANS)
    poses = [pose(t, [20 * np.cos(t), 20 * np.sin(t), 0.002 * i], 0.001 * i) for i, t in enumerate(theta)]
    return case([pts[cuts[i]:cuts[i + 1]] for i in range(MANY_SCANS)], poses if posed else None, np.array([-24.05, -24.02, -4.01], np.float32))


# ---- 4. many rays
@functools.lru_cache(maxsize=None)
def many_rays(extra):
    """one scan of 256 * 1024 + extra rays at truncation = voxel / 2: S = 1, three samples a ray.  extra = 1: 257 tiles of counts, so the
    lanes of the tile-sum scan take two tiles each; extra = 0: 256 tiles, one each, the last size of that path"""
    return case([shell(380 + extra, SCAN_LANES * SCAN_TILE + extra)], None, NEAR_ORIGIN, tau=VOXEL / 2)


# ---- 5. long runs and weights
LONG_RAYS, LONG_SCANS = 20000, 400


@functools.lru_cache(maxsize=None)
def long_runs(split):
    """20 000 rays whose endpoints lie in a ball two voxels across at range 2.  split: the same rays as 400 scans of 50, under poses that
    differ by a hundredth of a voxel"""
    rng = np.random.default_rng(390)
    d = rng.normal(size=(LONG_RAYS, 3))
    pts = (np.array([1.6, 1.0, 0.663]) + VOXEL * d / np.linalg.norm(d, axis=1)[:, None] * rng.uniform(0, 1, (LONG_RAYS, 1)) ** (1 / 3)).astype(np.float32)
    if not split:
        return case([pts], [pose(0.0, [0.0, 0.0, 0.0])], NEAR_ORIGIN)
    per = LONG_RAYS // LONG_SCANS
    poses = [pose(1e-4 * i, [1e-3 * np.cos(i), 1e-3 * np.sin(i), 1e-5 * i]) for i in range(LONG_SCANS)]
    return case([pts[i * per:(i + 1) * per] for i in range(LONG_SCANS)], poses, NEAR_ORIGIN)


STORED_WEIGHTS = (2.0 ** 24, 0.5, 1e-30, 3e38)
STORED_VALUES = (-1.0, -0.0, 1.0, 0.3333333)
CAP_TOTAL = np.float32(1.5)          # a stored 0.5 under one sample
CAPS = (CAP_TOTAL, np.nextafter(CAP_TOTAL, np.float32(0)), np.nextafter(CAP_TOTAL, np.float32(2)), np.float32(1e-3))


@functools.lru_cache(maxsize=None)
def weight_rays():
    """seven rays: four apart, and one three times over, whose voxels hold three samples"""
    pts = shell(395, 5, 1.5, 2.5)
    return frozen(np.concatenate([pts, pts[4:], pts[4:]]))


@functools.lru_cache(maxsize=None)
def weights(cap=None):
    """The rays of weight_rays over a stored map of exactly the voxels they touch, row i holding the weight STORED_WEIGHTS[i % 4] and the
    value STORED_VALUES[i // 4 % 4]: every pair of them lies under samples.  cap: max_weight, or None for none."""
    bare = R.integrate([weight_rays()], None, NEAR_ORIGIN, VOXEL, TAU)
    i = np.arange(len(bare[0]))
    stored = (bare[0], np.array(STORED_VALUES, np.float32)[i // 4 % 4], np.array(STORED_WEIGHTS, np.float32)[i % 4])
    return case([weight_rays()], None, NEAR_ORIGIN, map=stored, **({} if cap is None else dict(max_weight=float(cap))))


def weight_counts():
    """samples per stored row of weights()"""
    coord = R.samples([weight_rays()], None, NEAR_ORIGIN, VOXEL, TAU)[0]
    rows, count = np.unique(coord[:, ::-1], axis=0, return_counts=True)       # np.unique sorts by (cz, cy, cx): the map's order
    assert np.array_equal(rows[:, ::-1], weights()["map"][0])
    return count


CASES = {"wide": wide, "edge": edge, "far": far, "far_poses": far_poses, "many_scans": many_scans, "many_rays": many_rays, "long_runs": long_runs,
         "weights": weights}
# every fusion case, as (name, arguments)
FUSION = ([("wide", a) for a in WIDE_AXES] + [("edge", e) for e in (SORT_EXTENT, SORT_EXTENT + 1, MAX_EXTENT)] + [("far", s) for s in ("plus", "minus", "mixed")]
          + [("far_poses",), ("many_scans", True), ("many_scans", False), ("many_rays", 1), ("many_rays", 0), ("long_runs", False), ("long_runs", True),
             ("weights", None)] + [("weights", float(c)) for c in CAPS])
# the maps that go through the extraction and the ray cast
SURFACES = [("wide", a) for a in WIDE_AXES] + [("edge", e) for e in (SORT_EXTENT, SORT_EXTENT + 1, MAX_EXTENT)] + [("far", s) for s in ("plus", "minus", "mixed")] + [("far_poses",)]


def ident(key):
    return "-".join(str(k) for k in key)


# ---- the views of the ray cast
def into_sensor(T, world):
    """world points as directions in the frame of the sensor at pose T"""
    return ((np.asarray(world, np.float64) - T[:3, 3]) @ T[:3, :3]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def inside_dirs(name, *args):
    """per pose of a case: 150 of its scan's own rays, which pass through the voxels they made, and 100 directions anywhere"""
    c = CASES[name](*args)
    rng = np.random.default_rng(410)
    return [frozen(np.concatenate([s[:150], rng.normal(size=(100, 3)).astype(np.float32)])) for s in c["scans"]]


@functools.lru_cache(maxsize=None)
def gap_dirs(axes):
    """64 rays from the first sensor of a wide case at points of the second shell's surface beyond its sensor (seen from behind, the near
    half ends a ray without a hit), a little apart: across the gap"""
    c = wide(axes)
    xyz = R.extract(reference("wide", axes), c["origin"], c["voxel"])[0].astype(np.float64)
    t0, t1 = c["poses"][0][:3, 3], c["poses"][1][:3, 3]
    far_shell = xyz[(np.linalg.norm(xyz - t1, axis=1) < 3.5) & ((xyz - t1) @ (t1 - t0) > 0)]
    rng = np.random.default_rng(411)
    aim = far_shell[rng.choice(len(far_shell), 64, replace=False)] + 0.02 * rng.normal(size=(64, 3))
    return frozen(into_sensor(c["poses"][0], aim))


def gap_length(axes):
    c = wide(axes)
    return float(np.linalg.norm(c["poses"][1][:3, 3] - c["poses"][0][:3, 3]))
