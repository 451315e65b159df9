"""The restatement mi_knn_search is tested against (numpy, CPU): the whole n x m matrix of squared distances in float32, in either
distance arithmetic of mi_slam.h, packed into the keys (bits(d2) << 32) | j, sorted; the answer is the k smallest keys of every row.

MI_DIST_CPU_ROUNDING is float32 numpy in the stated order.  MI_DIST_FMA needs fma(a, a, c) = a * a + c rounded ONCE to float32, which
numpy does not have: the product of two float32 is exact in float64; the float64 sum is formed with its exact error (TwoSum) and, if
inexact, moved to the neighbour with an odd last bit (round to odd); one rounding of that to float32 is then the correctly rounded
result (53 >= 2 * 24 + 2 bits).  A plain float64 add followed by a cast rounds twice and is wrong in rare cases."""
import numpy as np

DIST_CPU_ROUNDING, DIST_FMA = 0, 1
KEY_EMPTY = np.uint64(0x7f800000ffffffff)     # d2 = +inf, idx = -1: what a slot without a candidate holds


def fma_sq_f32(a, c):
    """fma(a, a, c) for float32 arrays: the exact a * a + c, rounded once to float32."""
    a64, c64 = a.astype(np.float64), c.astype(np.float64)
    p = a64 * a64                                   # exact: 24 + 24 bits
    s = p + c64
    bb = s - p
    err = (p - (s - bb)) + (c64 - bb)               # TwoSum: p + c = s + err exactly
    even = (s.view(np.int64) & 1) == 0
    toward = np.where(err > 0, np.inf, -np.inf)
    s = np.where((err != 0) & even, np.nextafter(s, toward), s)      # round to odd
    return s.astype(np.float32)


def d2_matrix(query, cloud, dist_mode):
    """float32 [n, m]: |cloud[j] - query[i]|^2 in the arithmetic of dist_mode."""
    q = np.ascontiguousarray(query, np.float32)
    c = np.ascontiguousarray(cloud, np.float32)
    dx = c[None, :, 0] - q[:, None, 0]
    dy = c[None, :, 1] - q[:, None, 1]
    dz = c[None, :, 2] - q[:, None, 2]
    if dist_mode == DIST_CPU_ROUNDING:
        return (dx * dx + dy * dy) + dz * dz
    assert dist_mode == DIST_FMA
    return fma_sq_f32(dz, fma_sq_f32(dy, dx * dx))


def d2_pairs(a, b, dist_mode):
    """float32 [n]: |b[r] - a[r]|^2 over paired rows in the arithmetic of dist_mode -- d2_matrix's expression, operation for operation, so
    d2_pairs(q[i], c[j]) is d2_matrix(q, c)[i, j] bit for bit (tests/test_cluster_scale_reference.py)."""
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    dx = b[:, 0] - a[:, 0]
    dy = b[:, 1] - a[:, 1]
    dz = b[:, 2] - a[:, 2]
    if dist_mode == DIST_CPU_ROUNDING:
        return (dx * dx + dy * dy) + dz * dz
    assert dist_mode == DIST_FMA
    return fma_sq_f32(dz, fma_sq_f32(dy, dx * dx))


def sorted_keys(query, cloud, dist_mode, max_d2=np.inf, keep=32, block=256, only=None):
    """uint64 [n, keep]: every row's `keep` smallest keys, ascending, KEY_EMPTY where the candidates run out.  query None: self mode,
    the key of candidate i is void in row i (by index).  (Rows are worked `block` at a time: the matrix itself is never held whole.)
    only: the answer's rows `only` alone, [len(only), keep] -- what a large case can afford; in self mode its row r voids candidate only[r]."""
    self_mode = query is None
    cloud = np.ascontiguousarray(cloud, np.float32)
    query = cloud if self_mode else np.ascontiguousarray(query, np.float32)
    own = np.arange(len(query)) if only is None else np.asarray(only, np.int64)      # the caller's row of every row worked
    query = query[own]
    n, m = len(query), len(cloud)
    out = np.empty((n, keep), np.uint64)
    column = np.arange(m, dtype=np.uint64)[None, :]
    for lo in range(0, n, block):
        d2 = d2_matrix(query[lo:lo + block], cloud, dist_mode)
        rows = d2.shape[0]
        keys = (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | column
        if self_mode:
            keys[np.arange(rows), own[lo:lo + rows]] = KEY_EMPTY
        keys[d2 > np.float32(max_d2)] = KEY_EMPTY
        if m < keep:
            keys = np.concatenate([keys, np.full((rows, keep - m), KEY_EMPTY, np.uint64)], axis=1)
        elif m > keep:
            keys = np.partition(keys, keep - 1, axis=1)[:, :keep]
        out[lo:lo + rows] = np.sort(keys, axis=1)
    return out


def unpack(keys, k):
    """(idx int32 [n, k], d2 float32 [n, k], count int32 [n]) of the first k columns of sorted_keys."""
    keys = np.ascontiguousarray(keys[:, :k])
    idx = (keys & np.uint64(0xffffffff)).astype(np.uint32).view(np.int32)
    d2 = (keys >> np.uint64(32)).astype(np.uint32).view(np.float32)
    count = (keys != KEY_EMPTY).sum(axis=1).astype(np.int32)
    return idx, d2, count


def knn(query, cloud, k, dist_mode=DIST_CPU_ROUNDING, max_d2=np.inf):
    return unpack(sorted_keys(query, cloud, dist_mode, max_d2, keep=k), k)
