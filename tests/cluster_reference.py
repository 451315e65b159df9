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
The rows of the distance matrix are worked in blocks (the n x n matrix is never held whole) into the list of neighbour pairs, which
depends on the cloud, the radius and the arithmetic alone: a test that varies min_points or the size filter hands the same list back in."""
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


def _find(parent, x):
    while parent[x] != x:
        parent[x] = parent[parent[x]]
        x = parent[x]
    return x


def dbscan(cloud, radius, min_points=1, min_cluster_size=1, max_cluster_size=0, dist_mode=K.DIST_CPU_ROUNDING, pairs=None):
    """dict: labels int32 [n], n_clusters, sizes int32 [n_clusters], is_core uint8 [n], grouped int32 [n_grouped], and `raw`: every point's
    cluster before the size filter as the smallest core index of that cluster (-1: noise).  pairs: neighbour_pairs of the same cloud,
    radius and arithmetic, where the caller has them already."""
    n, i, j, key = neighbour_pairs(cloud, radius, dist_mode) if pairs is None else pairs
    core = 1 + np.bincount(i, minlength=n) >= min_points
    # the components of the core points: a plain union-find over the core-core edges, each taken once (j < i); the smaller root stays
    parent = list(range(n))
    edge = core[i] & core[j] & (j < i)
    for a, b in zip(i[edge].tolist(), j[edge].tolist()):
        ra, rb = _find(parent, a), _find(parent, b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    raw = np.full(n, -1, np.int64)
    for a in np.flatnonzero(core).tolist():
        raw[a] = _find(parent, a)                                     # the root is the smallest index of its set
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
