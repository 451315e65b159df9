"""float64 restatement of mi_voxel_downsample (the reference has no voxel filter, so this is the oracle of the voxel tests).

Voxel coordinates come from the float32 numpy expression floor((p - o) / float32(v)): one IEEE subtraction and one IEEE division,
the arithmetic include/mi_slam.h states for mi_voxel_index.  Voxels are grouped and ordered with np.lexsort((cx, cy, cz)) --
ascending by (cz, cy, cx), stable, so inside a voxel the points keep their index order -- and a voxel's point is the sequential
float64 sum of its points in index order, divided in float64 by their count and cast to float32."""
import numpy as np


def voxel_coords(xyz, voxel, origin):
    """int64 [n, 3]: floor((p - o) / float32(v)), every step in float32."""
    xyz = np.ascontiguousarray(xyz, np.float32)
    o = np.asarray(origin, np.float32).reshape(1, 3)
    q = np.floor((xyz - o) / np.float32(voxel))
    assert q.dtype == np.float32
    return q.astype(np.int64)


def downsample(xyz, voxel, origin=None):
    """-> centroids float32 [rows, 3], counts int32 [rows], coords int32 [rows, 3], voxel_of_point int32 [n].
    origin None: the per-axis minimum of the cloud."""
    xyz = np.ascontiguousarray(xyz, np.float32)
    n = len(xyz)
    origin = xyz.min(axis=0) if origin is None else np.asarray(origin, np.float32)
    c = voxel_coords(xyz, voxel, origin)
    order = np.lexsort((c[:, 0], c[:, 1], c[:, 2]))
    cs = c[order]
    head = np.ones(n, bool)
    head[1:] = (cs[1:] != cs[:-1]).any(axis=1)
    starts = np.flatnonzero(head)
    row_of_sorted = np.cumsum(head) - 1
    counts = np.diff(np.append(starts, n))
    voxel_of_point = np.empty(n, np.int32)
    voxel_of_point[order] = row_of_sorted
    sums = np.zeros((len(starts), 3), np.float64)
    x64 = xyz.astype(np.float64)
    # np.add.at adds unbuffered, one term after the other in the order given: inside every voxel that is index order (lexsort is stable)
    np.add.at(sums, voxel_of_point[order], x64[order])
    centroids = (sums / counts[:, None].astype(np.float64)).astype(np.float32)
    return centroids, counts.astype(np.int32), cs[starts].astype(np.int32), voxel_of_point
