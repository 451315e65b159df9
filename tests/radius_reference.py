"""The restatement mi_radius_search is tested against (numpy, CPU): tests/knn_reference.py's sorted keys of every row under the limit
r2 = radius * radius, formed in float32 as the library forms it, with as many columns as the cloud has points -- so a row is ALL its
members, ascending by (bits(d2) << 32) | j; the offsets are the running sum of the rows' lengths in int64."""
import numpy as np

import knn_reference as K


def r2_of(radius):
    """radius * radius as one IEEE float32 multiplication."""
    r = np.float32(radius)
    return np.float32(r * r)


def rows(query, cloud, radius, dist_mode=K.DIST_CPU_ROUNDING):
    """[uint64 array per query]: row i's keys, ascending.  query None: self mode, candidate i is void in row i (by index)."""
    cloud = np.ascontiguousarray(cloud, np.float32)
    keys = K.sorted_keys(query, cloud, dist_mode, max_d2=r2_of(radius), keep=len(cloud))
    return [row[row != K.KEY_EMPTY] for row in keys]


def csr(row_list):
    """(offsets int64 [n + 1], keys uint64 [total], total) of a list of rows."""
    lengths = np.array([len(r) for r in row_list], np.int64)
    offsets = np.concatenate([np.zeros(1, np.int64), np.cumsum(lengths)])
    keys = np.concatenate(row_list) if len(row_list) and offsets[-1] > 0 else np.zeros(0, np.uint64)
    return offsets, keys.astype(np.uint64), int(offsets[-1])


def unpack(keys):
    """(idx int32, d2 float32) of packed keys."""
    keys = np.ascontiguousarray(keys, np.uint64)
    return (keys & np.uint64(0xffffffff)).astype(np.uint32).view(np.int32), (keys >> np.uint64(32)).astype(np.uint32).view(np.float32)


def pack(idx, d2):
    """uint64 keys of (idx, d2) as the library returns them."""
    return (np.ascontiguousarray(d2, np.float32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.ascontiguousarray(idx, np.int32).view(np.uint32).astype(np.uint64)


def search(query, cloud, radius, dist_mode=K.DIST_CPU_ROUNDING):
    """(offsets, idx, d2, total): what mi_radius_search returns with sorted = 1."""
    offsets, keys, total = csr(rows(query, cloud, radius, dist_mode))
    idx, d2 = unpack(keys)
    return offsets, idx, d2, total
