"""The cases of tests/test_gpu_ndt_scale.py and what they share: clouds whose SORTED order is known run by run (K27's scan and fix-up at
the tile and wave edges), clouds at the sizes and extents where the voxel front takes its other paths, voxel maps made by hand (K30's
table and its look-up, voxel_table.hpp, at their limits) with their queries, the pose that sends a third of a cloud where voxel_axis refuses it -- and the numpy
restatements that tests/test_ndt_scale_regimes.py holds every case against, so that a case is shown to be what it is named for without a
device: the runs' starts and counts (ndt_reference.voxels), and, for the wrap map alone, the key, the hash and the capacity of
csrc/voxel_table.hpp.

No tolerance is introduced here: the matrices go through check_voxels and the sums through assert_sums / check_system of
tests/test_gpu_ndt.py with their bounds."""
import functools

import numpy as np

import ndt_reference as N
import plane_reference as P

TILE, WAVE = 256, 64                 # VOX_SUM_TILE (csrc/kernels.h): sorted positions per workgroup of K27's scan, one per lane; lanes per wave
FIXUP_LANES = 64                     # ndt_scatter_fixup_kernel: a lane adds the fronts of tiles first + 1 + lane, + 64, ...
SORT_ONE_PASS = 4096 * 64            # keys up to which the radix sort takes its small path (tests/test_gpu_sort.py)
MAX_EXTENT = 1 << 20                 # VOXEL_MAX_EXTENT, VOX_MAX_EXTENT: listed / occupied voxels per axis
PACKED_EXTENT = 1 << 10              # VOX_PACKED_EXTENT: up to here on every axis the voxel front sorts one packed key


def frozen(a):
    a.setflags(write=False)
    return a


def frozen_map(vox):
    for k in ("coord", "mean", "icov", "origin"):
        frozen(vox[k])
    return vox


def starts_of(count):
    """the sorted position every run begins at, from the runs' lengths in sorted order"""
    return np.concatenate([[0], np.cumsum(count)[:-1]]).astype(np.int64)


# ---- 1. run edges: one run per integer cx at voxel 1, origin 0, so the sorted order is the order of the list below
@functools.lru_cache(maxsize=None)
def run_edges():
    """(cloud float32 [n, 3], the runs' lengths in sorted order, {name: index of the first run of a named group}).  Fillers (6 points at
    least, so that they have a matrix of their own) bring a group to the lane it is to start on."""
    rng = np.random.default_rng(211)
    runs, named = [], {}

    def align(lane, modulo=TILE):
        need = (lane - sum(runs)) % modulo
        if need:
            runs.append(need if need >= 6 else need + modulo)

    def add(name, *lengths):
        named[name] = len(runs)
        runs.extend(lengths)

    add("a tile exactly", 256)                             # starts at tile_lo, ends on lane 255
    add("255 then 7", 255, 7)                              # ends on lane 254; the 7 start on lane 255 and cross the edge
    align(1)
    add("250, 7, 511", 250, 7, 511)                        # lanes 1 .. 250; 251 .. 255 and 0 .. 1; lane 2, a whole tile, and lane 0 of the next
    align(0)
    add("four waves", 64, 64, 64, 64)
    add("63, 130, 1", 63, 130, 1)                          # a wave less its last lane; from lane 63 over two wave edges; one point
    align(37)
    add("long", 16384 + 300)                               # enters 65 tiles: the fix-up's lane 0 takes a second trip
    while sum(runs) < 39000:
        runs.append(int(rng.integers(1, 700)))             # whatever alignment falls out
    align(200)
    add("to lane 255 from inside", 56)
    align(250)
    add("tail", 46)                                        # from lane 250 into the last, partial tile: n % 256 = 40
    lengths = np.array(runs, np.int64)
    cx = np.repeat(np.arange(len(lengths)), lengths)
    cloud = np.stack([cx + rng.uniform(0.05, 0.95, len(cx)), rng.uniform(0.05, 0.95, len(cx)), rng.uniform(0.05, 0.95, len(cx))], axis=1)
    return frozen(cloud[rng.permutation(len(cx))].astype(np.float32)), frozen(lengths), named


RUN_EDGES_VOXEL, RUN_EDGES_ORIGIN = 1.0, (0.0, 0.0, 0.0)


# ---- 2. size, sort paths and offset
OFFSET = (1000.0, -500.0, 250.0)
SORT_PATH_EXTENTS = ((1024, 1024, 1024), (1025, 1024, 1024), (5, 2000, 70000), (2 ** 20, 30, 30))      # tests/test_gpu_voxel.py::test_every_sort_path


@functools.lru_cache(maxsize=None)
def uniform_case(n, shifted=False):
    """(cloud, voxel, origin): n points uniform in [-5, 5]^3 at about 33 points per voxel.  The origin is set so that the first layer of
    voxels on every axis is a sliver 0.06 to 0.1 of a voxel thick: a few points each, most of them below min_points (no distribution),
    the rest so flat that the eigenvalue floor of 0.01 raises their smallest eigenvalue, which it does nowhere in the bulk."""
    rng = np.random.default_rng(223 + n)
    voxel = 0.5 if n > 200_000 else 0.8
    sliver = np.array([0.08, 0.06, 0.1]) * voxel
    cloud, origin = rng.uniform(-5, 5, (n, 3)), -5.0 - (voxel - sliver)
    if shifted:
        cloud, origin = cloud + np.array(OFFSET), origin + np.array(OFFSET)
    return frozen(cloud.astype(np.float32)), voxel, tuple(float(v) for v in origin.astype(np.float32))


@functools.lru_cache(maxsize=None)
def sort_path_case(which, turn):
    """(cloud, voxel 1, origin 0, the extents): 1 500 occupied voxels spread over SORT_PATH_EXTENTS[which] (turned `turn` places, as
    test_every_sort_path turns them) with 1 to 40 points each -- about 15 000 points; two voxels pin the longest extent to exactly its
    value.  A fifth of the voxels are flattened to 0.04 of a voxel along the SHORTEST extent (coordinates below 2^11 there: the grain of
    fp32 stays far below the thickness), so the floor of 0.01 has eigenvalues to raise."""
    extents = SORT_PATH_EXTENTS[which][turn:] + SORT_PATH_EXTENTS[which][:turn]
    rng = np.random.default_rng(227 + 3 * which + turn)
    long_axis, short_axis = int(np.argmax(extents)), int(np.argmin(extents))
    cells = np.stack([rng.integers(0, e, 1500) for e in extents], axis=1)
    cells[0, long_axis], cells[1, long_axis] = 0, extents[long_axis] - 1
    cells = np.unique(cells, axis=0)
    counts = rng.choice([1, 2, 5, 6, 7, 12, 40], len(cells))
    flat = rng.uniform(0, 1, len(cells)) < 0.2
    u = rng.uniform(0.05, 0.95, (int(counts.sum()), 3))
    flat_points = np.repeat(flat, counts)
    u[flat_points, short_axis] = 0.5 + 0.04 * (u[flat_points, short_axis] - 0.5)
    cloud = np.repeat(cells, counts, axis=0) + u
    return frozen(cloud[rng.permutation(len(cloud))].astype(np.float32)), 1.0, (0.0, 0.0, 0.0), extents


# ---- 3. maps made by hand
def hand_map(coords, voxel, origin, seed, holes=0):
    """A voxel map as mi_ndt_system takes it: the coordinates in strictly ascending (cz, cy, cx) order, mean = the voxel's centre plus a
    jitter below 0.4 voxel, icov = a random symmetric positive definite matrix of condition number 100 at most (eigenvalues 1 to 100 over
    voxel^2), both rounded to float32.  holes: every holes-th row is left without a distribution."""
    rng = np.random.default_rng(seed)
    coords = np.unique(np.asarray(coords, np.int64), axis=0)
    coords = coords[np.lexsort((coords[:, 0], coords[:, 1], coords[:, 2]))]
    nv = len(coords)
    origin = np.asarray(origin, np.float32)
    mean = (origin.astype(np.float64) + (coords + 0.5 + rng.uniform(-0.4, 0.4, (nv, 3))) * voxel).astype(np.float32)
    Q = np.linalg.qr(rng.normal(size=(nv, 3, 3)))[0]
    lam = 10.0 ** rng.uniform(0, 2, (nv, 3)) / voxel ** 2
    M = np.einsum("nai,ni,nbi->nab", Q, lam, Q)
    icov = np.stack([M[:, a, b] for a, b in N.TRI], axis=1).astype(np.float32)
    if holes:
        icov[::holes] = 0
    return frozen_map(dict(coord=coords.astype(np.int32), mean=mean, icov=icov, origin=origin, voxel=float(voxel)))


def map_queries(vox, seed, extra_cells=None):
    """The queries of a map, float32 [about 3 700, 3]: inside listed voxels; in the listed voxels ON each face of the listed box (their
    neighbour beyond the face is at rx = -1 or rx = ext) and in the cells one and two beyond them; around listed voxels up to two cells
    off (unlisted cells inside the box, more of the outside); anywhere in the box and two cells around it; and the cells the case adds."""
    rng = np.random.default_rng(seed)
    coord = vox["coord"].astype(np.int64)
    lo, hi = coord.min(axis=0), coord.max(axis=0)
    cells = [coord[rng.integers(0, len(coord), 1200)]]
    for a in range(3):
        for side, edge in ((-1, lo[a]), (1, hi[a])):
            on = coord[coord[:, a] == edge]
            on = on[rng.permutation(len(on))[:40]]
            for step in (0, 1, 2):
                c = on.copy()
                c[:, a] += side * step
                cells.append(c)
    cells.append(coord[rng.integers(0, len(coord), 1500)] + rng.integers(-2, 3, (1500, 3)))
    cells.append(rng.integers(lo - 2, hi + 3, (300, 3)))
    if extra_cells is not None:
        cells.append(np.asarray(extra_cells, np.int64))
    cells = np.concatenate(cells)
    q = vox["origin"].astype(np.float64) + (cells + rng.uniform(0.1, 0.9, cells.shape)) * vox["voxel"]
    return frozen(q[rng.permutation(len(q))].astype(np.float32))


COUNT_CASES = (1, 2, 3, 4, 1024, 1025)


def count_map(nv):
    """nv listed voxels around the origin of the lattice (so cmin is negative): up to four that touch face to face, or nv of the 2 197
    cells of a box; nv = 1025 with every seventh row left without a distribution"""
    rng = np.random.default_rng(229 + nv)
    if nv <= 4:
        cells = np.array([(-1, 0, 0), (0, 0, 0), (0, -1, 0), (0, 0, 1)])[:nv]
    else:
        cells = np.stack(np.meshgrid(*[np.arange(-6, 7)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
        cells = cells[rng.permutation(len(cells))[:nv]]
    vox = hand_map(cells, 0.8, (0.3, 0.1, -0.2), 233 + nv, holes=7 if nv == 1025 else 0)
    return vox, map_queries(vox, 239 + nv)


def slab_map(axis):
    """A map that spans exactly 2^20 voxels along `axis`, from -2^19 to 2^19 - 1: eight layers at either end, four in the middle, 8 x 8
    cells per layer (from -3 to 4: cmin is negative on every axis), nine in ten of them listed.  Voxel 1, origin 0: a position up there
    is an integer plus a fraction of 1 / 32, exact in fp32."""
    rng = np.random.default_rng(241 + axis)
    s = np.concatenate([np.arange(-2 ** 19, -2 ** 19 + 8), np.arange(0, 4), np.arange(2 ** 19 - 8, 2 ** 19)])
    others = np.arange(-3, 5)
    grid = np.stack(np.meshgrid(s, others, others, indexing="ij"), axis=-1).reshape(-1, 3)
    grid = grid[rng.uniform(0, 1, len(grid)) < 0.9]
    cells = np.empty_like(grid)
    cells[:, axis], cells[:, (axis + 1) % 3], cells[:, (axis + 2) % 3] = grid[:, 0], grid[:, 1], grid[:, 2]
    vox = hand_map(cells, 1.0, (0.0, 0.0, 0.0), 251 + axis)
    return vox, map_queries(vox, 257 + axis)


FAR_LOW = -2 ** 30 + 8                # the lowest listed coordinate of far_map


def far_map(axis):
    """A map whose lowest coordinate along `axis` is -2^30 + 8, eight above the least one mi_voxel_index gives.  Down there
    floor((p - o) / v) in fp32 is a multiple of 64 whatever the voxel size, so a point's OWN voxel is -2^30 + 64 k; the listed voxels are
    those for k = 1 .. 12 and the ones either side of them (reached as neighbours, by integer arithmetic on the index), and the lowest
    one.  Voxel 0.5, origin 0: |p| stays below 2^29, far below the 1e18 the input check admits.  Queries are added at k = 0 (the least
    index there is: its neighbour at -2^30 - 1 is formed in the lookup) and at k = 13, 14 (beyond the listed box)."""
    rng = np.random.default_rng(263 + axis)
    s = np.concatenate([[FAR_LOW], (-2 ** 30 + 64 * np.arange(1, 13)[:, None] + np.array([-1, 0, 1])).ravel()])
    others = np.arange(-2, 4)
    grid = np.stack(np.meshgrid(s, others, others, indexing="ij"), axis=-1).reshape(-1, 3)
    grid = grid[(rng.uniform(0, 1, len(grid)) < 0.5) | (grid[:, 0] == FAR_LOW)]
    extra = np.stack(np.meshgrid(-2 ** 30 + 64 * np.array([0, 13, 14]), np.arange(-4, 6), np.arange(-4, 6), indexing="ij"), axis=-1).reshape(-1, 3)

    def turned(g):
        c = np.empty_like(g)
        c[:, axis], c[:, (axis + 1) % 3], c[:, (axis + 2) % 3] = g[:, 0], g[:, 1], g[:, 2]
        return c

    vox = hand_map(turned(grid), 0.5, (0.0, 0.0, 0.0), 269 + axis)
    return vox, map_queries(vox, 271 + axis, turned(extra))


# the table, restated for the wrap map alone: voxel_table.hpp's voxel_key, voxel_hash and voxel_table_slots(nv, 2)
# (tests/test_voxel_table.py holds the header itself against these, on the host)
def table_keys(coord, shifts=(0, 20, 40), cmin=None):
    """the keys of voxel coordinates inside the listed box; cmin None: the coordinates are the list itself"""
    rel = np.asarray(coord, np.int64) - (np.asarray(coord, np.int64).min(axis=0) if cmin is None else np.asarray(cmin, np.int64))
    assert (rel >= 0).all() and (rel < MAX_EXTENT).all()
    rel = rel.astype(np.uint64)
    return (rel[:, 0] << np.uint64(shifts[0])) | (rel[:, 1] << np.uint64(shifts[1])) | (rel[:, 2] << np.uint64(shifts[2]))


def table_hash(key):
    """splitmix64's finaliser on uint64 arrays (the products wrap)"""
    key = np.array(key, np.uint64)
    key ^= key >> np.uint64(30)
    key *= np.uint64(0xbf58476d1ce4e5b9)
    key ^= key >> np.uint64(27)
    key *= np.uint64(0x94d049bb133111eb)
    return key ^ (key >> np.uint64(31))


def table_capacity(nv):
    capacity = 2
    while capacity < 2 * nv:
        capacity <<= 1
    return capacity


def table_build(vox, order):
    """the table after the rows with a distribution arrived in `order` -> (slot of every row or -1, how many rows went past the last slot)"""
    keys, mask = table_keys(vox["coord"]), table_capacity(len(vox["coord"])) - 1
    home = (table_hash(keys) & np.uint64(mask)).astype(np.int64)
    taken, slot_of, wrapped = {}, np.full(len(keys), -1, np.int64), 0
    has = N.has_distribution(vox)
    for row in order:
        if not has[row]:
            continue
        slot = int(home[row])
        while slot in taken:
            wrapped += slot == mask
            slot = (slot + 1) & mask
        taken[slot] = row
        slot_of[row] = slot
    return slot_of, wrapped


WRAP_SIDE, WRAP_NV, WRAP_BASE = 40, 1000, (-7, -11, -13)


@functools.lru_cache(maxsize=None)
def wrap_map():
    """(map, queries, the rows whose home slot is the table's last one): 1 000 of the 64 000 cells of a box, its two far corners among them
    (they fix cmin and so every key), four of them chosen by a search for keys that hash to slot `mask`; the queries visit every cell
    of the box that hashes there, listed or not, so that lookups of absent keys wrap too."""
    rng = np.random.default_rng(277)
    g = np.arange(WRAP_SIDE)
    cells = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    mask = table_capacity(WRAP_NV) - 1
    at_mask = np.flatnonzero((table_hash(table_keys(cells, cmin=(0, 0, 0))) & np.uint64(mask)) == np.uint64(mask))
    corners = np.flatnonzero((cells == 0).all(axis=1) | (cells == WRAP_SIDE - 1).all(axis=1))
    chosen = np.setdiff1d(at_mask, corners)[:4]
    rest = np.setdiff1d(np.arange(len(cells)), np.concatenate([at_mask, corners]))
    listed = np.concatenate([chosen, corners, rest[rng.permutation(len(rest))[:WRAP_NV - len(chosen) - len(corners)]]])
    vox = hand_map(cells[listed] + np.array(WRAP_BASE), 0.8, (0.3, 0.1, -0.2), 281)
    wrap_cells = cells[chosen] + np.array(WRAP_BASE)
    rows = np.flatnonzero((vox["coord"][:, None, :] == wrap_cells[None]).all(axis=2).any(axis=1))
    return vox, map_queries(vox, 283, cells[at_mask] + np.array(WRAP_BASE)), frozen(rows)


MAP_CASES = tuple(["count %d" % nv for nv in COUNT_CASES] + ["slab %s" % a for a in "xyz"] + ["far %s" % a for a in "xyz"] + ["wrap"])
NEIGHBOURHOODS = (1, 7, 27)


@functools.lru_cache(maxsize=None)
def map_case(name):
    """(map, queries) of a name in MAP_CASES"""
    kind, _, arg = name.partition(" ")
    if kind == "count":
        return count_map(int(arg))
    if kind == "slab":
        return slab_map("xyz".index(arg))
    if kind == "far":
        return far_map("xyz".index(arg))
    assert name == "wrap"
    return wrap_map()[:2]


@functools.lru_cache(maxsize=None)
def map_lookup(name):
    return N.Lookup(map_case(name)[0])


@functools.lru_cache(maxsize=None)
def map_reference(name, neighbourhood):
    """ndt_reference.sums_at of the case's queries, worked once"""
    vox, queries = map_case(name)
    return N.sums_at(queries, vox, neighbourhood, lookup=map_lookup(name))


# ---- 4. positions voxel_axis refuses
REFUSED_SHIFT = 64.0


def refused_case(moving, vox):
    """(cloud float32 [n, 3], T float32 [4, 4], the rows sent out of range) from a scene's moving cloud and its map at voxel 0.5: T is a
    rotation of one degree about x (which leaves x as it is) and a translation of (64, 0.02, -0.03); two of three points are the scene's
    own, moved by the inverse of T, so that T brings them back onto the map; every third has x = 2^29 - 64, which the input check and
    mi_voxel_index admit -- (x - o) / 0.5 rounds to 2^30 - 128 -- and which T moves to 2^29: (2^29 - o) / 0.5 rounds to 2^30, refused."""
    assert vox["voxel"] == 0.5 and -4 < vox["origin"][0] < 0
    R, t = P.rodrigues([np.deg2rad(1.0), 0.0, 0.0]), np.array([REFUSED_SHIFT, 0.02, -0.03])
    cloud = ((moving.astype(np.float64) - t) @ R).astype(np.float32)                # R^T (p - t), row vectors
    out = np.arange(0, len(cloud), 3)
    cloud[out, 0] = np.float32(2.0 ** 29 - 64)
    return frozen(cloud), frozen(P.pose44(R, t)), frozen(out)
