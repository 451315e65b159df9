"""The restatement mi_estimate_normals is tested against (numpy, CPU, float64).  The neighbour sets are those of the k-NN restatement in
self mode (tests/knn_reference.py: point i skipped by index, duplicates kept); per point the covariance of the neighbourhood's
count + 1 points -- the point itself and its neighbours -- about their mean, divided by the number of points, in the two-pass form
(mean first, then the centred products), and numpy.linalg.eigh of it."""
import numpy as np

import knn_reference as K


def from_neighbours(cloud, idx):
    """(lambda [n, 3] ascending, normal [n, 3] float64 unit with arbitrary sign, C [n, 3, 3], count [n] int32) from the neighbour
    lists idx [n, k] (-1: no neighbour in that slot)."""
    p = np.ascontiguousarray(cloud, np.float32).astype(np.float64)
    n = len(p)
    have = idx >= 0
    pts = np.concatenate([p[:, None, :], p[np.where(have, idx, 0)]], axis=1)             # [n, k + 1, 3]: the point itself first
    w = np.concatenate([np.ones((n, 1)), have.astype(np.float64)], axis=1)[:, :, None]
    c = w.sum(axis=1)                                                                    # [n, 1] = count + 1
    mean = (pts * w).sum(axis=1) / c
    d = (pts - mean[:, None, :]) * w
    C = np.einsum("nki,nkj->nij", d, d) / c[:, :, None]
    C = (C + np.transpose(C, (0, 2, 1))) / 2.0
    lam, V = np.linalg.eigh(C)
    return lam, np.ascontiguousarray(V[:, :, 0]), C, have.sum(axis=1).astype(np.int32)


def normals(cloud, k, dist_mode=K.DIST_CPU_ROUNDING, max_d2=np.inf):
    idx, _, _ = K.knn(None, cloud, k, dist_mode, max_d2)
    return from_neighbours(cloud, idx)


def curvature(lam):
    """lambda0 / (lambda0 + lambda1 + lambda2) with lambda0 clamped below at 0; 0 where the sum is not positive"""
    total = lam.sum(axis=1)
    return np.where(total > 0, np.maximum(lam[:, 0], 0.0) / np.where(total > 0, total, 1.0), 0.0)
