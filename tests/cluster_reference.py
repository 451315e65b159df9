"""The restatement mi_cluster_dbscan is tested against (numpy, CPU), on knn_reference.d2_matrix: that function emulates both distance
arithmetics of mi_slam.h bit for bit, so the neighbour graph here is the device's and every comparison with it is integer equality.

The rules, as include/mi_slam.h states them:
  neighbours   j != i with d2(i, j) <= r2, r2 = radius * radius in one float32 multiplication; a point AT the radius belongs
  core         1 + #neighbours >= min_points
  clusters     connected components of the core points under "is a neighbour of" (a plain union-find over the core-core edges)
  border       not core, at least one core neighbour: the cluster of the core neighbour with the smallest key (bits(d2) << 32) | j
  noise        the rest: -1
  size filter  a cluster's size counts core and border points; outside [min_cluster_size, max_cluster_size] (0: no upper limit) it is
               dissolved to -1; is_core is not affected
  numbering    the survivors 0 .. n_clusters - 1 by ascending smallest core member index
  grouped      the labelled points sorted by (label, index)
Everything starts from the list of neighbour pairs, which depends on the cloud, the radius and the arithmetic alone: a test that varies
min_points or the size filter hands the same list back in.  There are two ways to it:
  neighbour_pairs          the rows of the distance matrix, worked in blocks (the n x n matrix is never held whole): O(n^2) time, the
                           plainest statement, what tests/test_gpu_cluster.py uses up to 5 000 points
  neighbour_pairs_binned   the candidates of the 27 host-side bins around each point, filtered by the same emulated distance per pair
                           (K.d2_pairs): what the 10^5-point clouds of tests/test_gpu_cluster_scale.py can afford
and two ways from the core-core edges to the components: the Python union-find and scipy's connected_components (dbscan(components=...)).
tests/test_cluster_scale_reference.py holds the two pair lists equal, all four arrays in order, and the two components' outputs equal, on
every cloud of the small suite and on prefixes of the large ones, in both arithmetics."""
import numpy as np

import knn_reference as K

KEY_NONE = np.uint64(0xffffffffffffffff)


def neighbour_pairs(cloud, radius, dist_mode=K.DIST_CPU_ROUNDING, block=512):
    """(n, i, j, key): every ordered pair i != j with d2(i, j) <= r2, by ascending (i, j), and its key (bits(d2) << 32) | j"""
    cloud = np.ascontiguousarray(cloud, np.float32)
    n = len(cloud)
    r2 = np.float32(radius) * np.float32(radius)
    rows, cols, keys = [], [], []
    for lo in range(0, n, block):
        d2 = K.d2_matrix(cloud[lo:lo + block], cloud, dist_mode)
        near = d2 <= r2
        near[np.arange(near.shape[0]), np.arange(lo, lo + near.shape[0])] = False
        a, b = np.nonzero(near)
        rows.append(a + lo)
        cols.append(b)
        keys.append((d2[a, b].view(np.uint32).astype(np.uint64) << np.uint64(32)) | b.astype(np.uint64))
    return n, np.concatenate(rows), np.concatenate(cols), np.concatenate(keys)


BIN_SLACK = 1e-5          # the bins' edge over the radius: far above the 3e-7 by which fp32 rounding can let a pair in (below)
BIN_MAX_DIM = 1 << 20     # bins per axis at most (the edge grows where the box asks for more): three of them pack into an int64


def neighbour_pairs_binned(cloud, radius, dist_mode=K.DIST_CPU_ROUNDING):
    """neighbour_pairs -- the same (n, i, j, key) in the same order -- in O(n) memory: the candidates of a point are the points of the 27
    bins around its own, and K.d2_pairs, the emulated fp32 distance, decides among them exactly as d2_matrix does in neighbour_pairs.

    The bins are the host's own (float64, plain numpy: a stable argsort of the bin codes and searchsorted); nothing of the device's grid is
    restated.  They only have to yield a superset: d2 <= r2 in fp32 means every |dx| <= radius (1 + 3e-7) (fl(dx) is within 2^-24 of dx, the
    sum is at least fl(dx)^2 (1 - 2^-24) and r2 at most radius^2 (1 + 2^-24), squares far above the subnormals), and two coordinates less than
    one edge = radius (1 + BIN_SLACK) apart lie in the same bin or in adjacent ones."""
    cloud = np.ascontiguousarray(cloud, np.float32)
    n = len(cloud)
    r2 = np.float32(radius) * np.float32(radius)
    assert r2 >= 2.0 ** -100, "the superset argument needs squares far above fp32's subnormals"
    p = cloud.astype(np.float64)
    low = p.min(axis=0)
    edge = max(float(np.float32(radius)) * (1 + BIN_SLACK), float((p.max(axis=0) - low).max()) / BIN_MAX_DIM)
    cell = np.floor((p - low) / edge).astype(np.int64) + 1                    # (+ 1: a ring of empty bins, so that no neighbour code wraps)
    ny, nz = (int(v) + 2 for v in cell.max(axis=0)[1:])
    code = (cell[:, 0] * ny + cell[:, 1]) * nz + cell[:, 2]
    order = np.argsort(code, kind="stable")
    ordered = code[order]
    rows, cols, dist = [], [], []
    for step in np.ndindex(3, 3, 3):
        there = code + (((step[0] - 1) * ny + (step[1] - 1)) * nz + (step[2] - 1))
        first = np.searchsorted(ordered, there, side="left")
        count = np.searchsorted(ordered, there, side="right") - first
        a = np.repeat(np.arange(n), count)
        b = order[np.repeat(first - (np.cumsum(count) - count), count) + np.arange(len(a))]
        a, b = a[a != b], b[a != b]
        d2 = K.d2_pairs(cloud[a], cloud[b], dist_mode)
        near = d2 <= r2
        rows.append(a[near])
        cols.append(b[near])
        dist.append(d2[near])
    i, j, d2 = np.concatenate(rows), np.concatenate(cols), np.concatenate(dist)
    by = np.argsort(i * n + j)                                                # ascending (i, j); no pair twice: every point is in one bin
    i, j = i[by], j[by]
    return n, i, j, (d2[by].view(np.uint32).astype(np.uint64) << np.uint64(32)) | j.astype(np.uint64)


def _find(parent, x):
    while parent[x] != x:
        parent[x] = parent[parent[x]]
        x = parent[x]
    return x


def _roots_union_find(n, a, b):
    """the root (smallest index) of every point's set under the edges (a[e], b[e]): a plain union-find in Python, the smaller root stays"""
    parent = list(range(n))
    for x, y in zip(a.tolist(), b.tolist()):
        rx, ry = _find(parent, x), _find(parent, y)
        if rx != ry:
            parent[max(rx, ry)] = min(rx, ry)
    return np.array([_find(parent, x) for x in range(n)], np.int64)


def _roots_scipy(n, a, b):
    """the same roots from scipy.sparse.csgraph.connected_components: the minimum index per component (what a large cloud can afford)"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    graph = coo_matrix((np.ones(len(a), np.int8), (a, b)), shape=(n, n)).tocsr()
    count, component = connected_components(graph, directed=False)
    smallest = np.full(count, n, np.int64)
    np.minimum.at(smallest, component, np.arange(n))
    return smallest[component]


COMPONENTS = {"union-find": _roots_union_find, "scipy": _roots_scipy}


def dbscan(cloud, radius, min_points=1, min_cluster_size=1, max_cluster_size=0, dist_mode=K.DIST_CPU_ROUNDING, pairs=None, components="union-find"):
    """dict: labels int32 [n], n_clusters, sizes int32 [n_clusters], is_core uint8 [n], grouped int32 [n_grouped], and `raw`: every point's
    cluster before the size filter as the smallest core index of that cluster (-1: noise).  pairs: neighbour_pairs (or
    neighbour_pairs_binned) of the same cloud, radius and arithmetic, where the caller has them already.  components: which of COMPONENTS
    finds the sets of the core points; both give the same roots (tests/test_cluster_scale_reference.py)."""
    n, i, j, key = neighbour_pairs(cloud, radius, dist_mode) if pairs is None else pairs
    core = 1 + np.bincount(i, minlength=n) >= min_points
    # the components of the core points over the core-core edges, each taken once (j < i); the root of a set is its smallest index
    edge = core[i] & core[j] & (j < i)
    roots = COMPONENTS[components](n, i[edge], j[edge])
    raw = np.where(core, roots, -1)                                   # (a point that is not core has no edge: it is its own root here)
    # the border rule: the smallest key over the core neighbours of a point that is not core
    best = np.full(n, KEY_NONE, np.uint64)
    reach = ~core[i] & core[j]
    np.minimum.at(best, i[reach], key[reach])
    border = np.flatnonzero(best != KEY_NONE)
    raw[border] = raw[(best[border] & np.uint64(0xffffffff)).astype(np.int64)]
    # the size filter and the numbering
    roots, sizes = np.unique(raw[raw >= 0], return_counts=True)       # ascending roots = ascending smallest core index
    keep = (sizes >= min_cluster_size) & ((max_cluster_size == 0) | (sizes <= max_cluster_size))
    rank = np.full(n, -1, np.int64)
    rank[roots[keep]] = np.arange(int(keep.sum()))
    labels = np.where(raw >= 0, rank[np.maximum(raw, 0)], -1).astype(np.int32)
    labelled = np.flatnonzero(labels >= 0)
    grouped = labelled[np.argsort(labels[labelled], kind="stable")].astype(np.int32)
    return {"labels": labels, "n_clusters": int(keep.sum()), "sizes": sizes[keep].astype(np.int32), "is_core": core.astype(np.uint8),
            "grouped": grouped, "raw": raw}
