"""The cases of tests/test_gpu_cluster_scale.py and what they share: the clouds that take mi_cluster_dbscan beyond the 5 000 points of
tests/test_gpu_cluster.py, and their restatements (tests/cluster_reference.py: the binned pair list, scipy's components), built once per
parameter set and handed out frozen.  tests/test_cluster_scale_reference.py holds every case against the regime it is named for, on the
restatement and on the restated plan of tests/search_scale_cases.py (grid_plan, radius_points_per_cell) alone, no device needed.

  thinned      a seeded 45 % of the 65 x 64 x 64 integer lattice in shuffled order, radius 1: every squared distance is a small integer,
               exact in both arithmetics.  At min_points 4: thousands of clusters (the grouping's 20-bit sort), one of tens of thousands of
               points, noise, and border points whose nearest core neighbours lie in different clusters at d2 = 1 -- the index decides
  scene        120 000 float32 points: 36 Gaussian blobs and uniform noise, radius 0.3; the two arithmetics differ in their last bit
  long_chain   100 000 points one apart along x in ascending, descending and shuffled index order: one set whose parent list can be as
               deep as the cloud (ascending: every lane hooks under its predecessor at once), over a grid of one clamped axis
  singletons   the first 2^20 + 1 sites of a 102^3 lattice in raster order, shuffled.  Below radius 1 every point is its own cluster
               (n_clusters > 2^20: the grouping's 30-bit sort), at radius 1 all are one set; both answers are analytic

Compaction tiles (1024 flags each; the one-workgroup tile scan takes two tiles per lane from 257 tiles on): `singletons` has 1025, the
other clouds 98 to 118."""
import functools

import numpy as np

import cluster_reference as R
import knn_reference as K
import search_scale_cases as S

MODES = (K.DIST_CPU_ROUNDING, K.DIST_FMA)
BELOW_ONE = float(np.nextafter(np.float32(1), np.float32(0)))
COMPACT_TILE = 1024                  # OUTLIER_SCAN_TILE of csrc/kernels.h
SORT_BITS = 10                       # the grouping's sort takes 10, 20 or 30 bits: the first width that holds n_clusters (csrc/cluster_api.hip)

THINNED_SIDES, THINNED_SHARE, THINNED_SEED = (65, 64, 64), 0.45, 11
THINNED_RADIUS, THINNED_MIN_POINTS = 1.0, 4
# (min_points, min_cluster_size, max_cluster_size): the workhorse; every point core; a filter that dissolves the giant and the singletons
THINNED_RUNS = ((THINNED_MIN_POINTS, 1, 0), (1, 1, 0), (THINNED_MIN_POINTS, 2, 1000))
SCENE_POINTS, SCENE_BLOBS, SCENE_SEED = 120_000, 36, 29
SCENE_RADIUS, SCENE_MIN_POINTS = 0.3, (1, 5, 12)
SCENE_FINE_PPC = "0.25"              # MISLAM_KNN_POINTS_PER_CELL at which the scene's grid has 64 and more cells per axis
CHAIN_POINTS, CHAIN_ORDERS, CHAIN_SEED = 100_000, ("ascending", "descending", "shuffled"), 31
# (radius, min_points): one set; one set whose two ends are border points; every point alone
CHAIN_RUNS = ((1.0, 1), (1.0, 3), (BELOW_ONE, 1))
SINGLETONS_SIDE, SINGLETONS_POINTS, SINGLETONS_SEED = 102, (1 << 20) + 1, 37


def frozen(a):
    a.setflags(write=False)
    return a


def sort_bits(n_clusters):
    """the width cluster_api.hip picks for the (label, index) sort"""
    bits = SORT_BITS
    while bits < 30 and (1 << bits) < n_clusters:
        bits += SORT_BITS
    return bits


def compact_tiles(n):
    return (n + COMPACT_TILE - 1) // COMPACT_TILE


def lattice_sites(nx, ny, nz):
    """the integer lattice in raster order, x fastest: float32 [nx ny nz, 3]"""
    z, y, x = np.meshgrid(np.arange(nz, dtype=np.float32), np.arange(ny, dtype=np.float32), np.arange(nx, dtype=np.float32), indexing="ij")
    return np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1)


def raster_prefix(side, count, seed):
    """the first `count` sites of the side^3 lattice in raster order (a connected set: whole layers, whole rows, one partial row), shuffled"""
    return lattice_sites(side, side, side)[:count][np.random.default_rng(seed).permutation(count)]


def prefix_answer(n, together):
    """mi_cluster_dbscan's answer on a raster prefix with min_points 1: at radius 1 one cluster of everything, below it every point alone"""
    every = np.arange(n, dtype=np.int32)
    if together:
        return {"labels": np.zeros(n, np.int32), "n_clusters": 1, "sizes": np.array([n], np.int32), "is_core": np.ones(n, np.uint8), "grouped": every}
    return {"labels": every, "n_clusters": n, "sizes": np.ones(n, np.int32), "is_core": np.ones(n, np.uint8), "grouped": every}


def make_thinned():
    sites = lattice_sites(*THINNED_SIDES)
    return sites[np.random.default_rng(THINNED_SEED).permutation(len(sites))[:int(THINNED_SHARE * len(sites))]]


def make_scene():
    rng = np.random.default_rng(SCENE_SEED)
    centres, spread = rng.uniform(-40, 40, (SCENE_BLOBS, 3)), rng.uniform(0.5, 1.5, SCENE_BLOBS)
    per_blob = 3000
    blobs = [c + s * rng.normal(size=(per_blob, 3)) for c, s in zip(centres, spread)]
    noise = rng.uniform(-45, 45, (SCENE_POINTS - per_blob * SCENE_BLOBS, 3))
    return np.concatenate(blobs + [noise])[rng.permutation(SCENE_POINTS)].astype(np.float32)


def make_chain(order):
    x = np.arange(CHAIN_POINTS, dtype=np.float32)
    x = {"ascending": x, "descending": x[::-1], "shuffled": x[np.random.default_rng(CHAIN_SEED).permutation(CHAIN_POINTS)]}[order]
    chain = np.zeros((CHAIN_POINTS, 3), np.float32)
    chain[:, 0] = x
    return chain


@functools.lru_cache(maxsize=None)
def cloud(name):
    """"thinned", "scene", "chain ascending" / "chain descending" / "chain shuffled", "singletons": float32 [n, 3], frozen"""
    if name.startswith("chain "):
        return frozen(make_chain(name[6:]))
    if name == "singletons":
        return frozen(raster_prefix(SINGLETONS_SIDE, SINGLETONS_POINTS, SINGLETONS_SEED))
    return frozen({"thinned": make_thinned, "scene": make_scene}[name]())


@functools.lru_cache(maxsize=None)
def pairs(name, radius, mode):
    """the binned neighbour pairs of a cloud: one pass for every min_points and size filter"""
    return tuple(v if isinstance(v, int) else frozen(v) for v in R.neighbour_pairs_binned(cloud(name), radius, mode))


@functools.lru_cache(maxsize=None)
def reference(name, radius, min_points, min_size, max_size, mode):
    ref = R.dbscan(cloud(name), radius, min_points, min_size, max_size, mode, pairs=pairs(name, radius, mode), components="scipy")
    return {k: (frozen(v) if isinstance(v, np.ndarray) else v) for k, v in ref.items()}


def tied_borders(pair_list, ref):
    """the border points whose core neighbours at the smallest distance lie in more than one cluster (`raw`, before the size filter): the
    points at which only the index half of the border key decides"""
    n, i, j, key = pair_list
    core = ref["is_core"] == 1
    reach = ~core[i] & core[j]
    i, j, bits = i[reach], j[reach], key[reach] >> np.uint64(32)
    nearest = np.full(n, np.uint64(0xffffffff), np.uint64)
    np.minimum.at(nearest, i, bits)
    at = bits == nearest[i]
    i, root = i[at], ref["raw"][j[at]]
    lowest, highest = np.full(n, n, np.int64), np.full(n, -1, np.int64)
    np.minimum.at(lowest, i, root)
    np.maximum.at(highest, i, root)
    return np.flatnonzero(highest > lowest)


def plan(points, radius, knn_points_per_cell=None):
    """the grid mi_cluster_dbscan plans over `points`: search_scale_cases.grid_plan at the radius rule's points per cell, or at the
    MISLAM_KNN_POINTS_PER_CELL that overrides it -> (dims, inv_h, raised)"""
    ppc = float(knn_points_per_cell) if knn_points_per_cell is not None else S.radius_points_per_cell(points, radius)[0]
    return S.grid_plan(points, ppc)
