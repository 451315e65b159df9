"""The restatement mi_iss_keypoints is tested against (numpy, CPU), built on tests/knn_reference.py, as include/mi_slam.h states the rules:

  balls      r2 = float32(radius) * float32(radius); { j != i (by index) : d2(i, j) <= r2 } with d2 the float32 matrix of
             knn_reference.d2_matrix in the arithmetic of dist_mode
  scatter    d = float64(p_j) - float64(p_i); S = sum d, Q = sum d d^T over the salient ball; c = count + 1; m = S / c;
             C = Q / c - m m^T (numpy's summation order, not the device's: the tests' bound covers the difference)
  lambda     numpy.linalg.eigvalsh(C), ascending
  gate       count >= min_neighbours and lambda1 < float64(float32(gamma_21)) * lambda2 and lambda0 < float64(float32(gamma_32)) * lambda1
  saliency   max(float32(lambda0), 0) where the gate holds, +0 elsewhere
  nms        of a GIVEN float32 saliency array: i is a keypoint iff saliency[i] > 0, its non-max ball holds at least min_neighbours
             points, and every j in it has saliency[j] < saliency[i], or saliency[j] == saliency[i] and j > i"""
import numpy as np

import knn_reference as K


def _balls(cloud, radius, dist_mode, own, lo, block):
    """bool [rows, n]: row r holds the ball of point own[lo + r], itself left out by index"""
    r2 = np.float32(radius) * np.float32(radius)
    rows = own[lo:lo + block]
    inside = K.d2_matrix(cloud[rows], cloud, dist_mode) <= r2
    inside[np.arange(len(rows)), rows] = False
    return inside


def saliency(cloud, salient_radius, dist_mode, gamma_21=0.975, gamma_32=0.975, min_neighbours=5, block=256, only=None):
    """dict of per-point results (of the points `only` alone where given -- what a large case can afford):
    count int32 [n]; lam float64 [n, 3] ascending; gate bool [n]; saliency float32 [n]; margin float64 [n]: how far the nearer of the
    two ratio tests is from its gamma, |lambda1 - g21 lambda2| / lambda2 and |lambda0 - g32 lambda1| / lambda1 (0 where the divisor is
    not positive)."""
    cloud = np.ascontiguousarray(cloud, np.float32)
    c64 = cloud.astype(np.float64)
    own = np.arange(len(cloud)) if only is None else np.asarray(only, np.int64)
    g21, g32 = np.float64(np.float32(gamma_21)), np.float64(np.float32(gamma_32))
    n = len(own)
    count, lam = np.empty(n, np.int32), np.empty((n, 3), np.float64)
    for lo in range(0, n, block):
        inside = _balls(cloud, salient_radius, dist_mode, own, lo, block)
        rows = inside.shape[0]
        d = (c64[None, :, :] - c64[own[lo:lo + rows]][:, None, :]) * inside[:, :, None]      # (0 outside the ball)
        cnt = inside.sum(axis=1)
        c = (cnt + 1).astype(np.float64)
        m = d.sum(axis=1) / c[:, None]
        q = np.einsum("rja,rjb->rab", d, d)
        cov = q / c[:, None, None] - m[:, :, None] * m[:, None, :]
        count[lo:lo + rows] = cnt
        lam[lo:lo + rows] = np.linalg.eigvalsh(cov)
    l0, l1, l2 = lam[:, 0], lam[:, 1], lam[:, 2]
    gate = (count >= min_neighbours) & (l1 < g21 * l2) & (l0 < g32 * l1)
    with np.errstate(divide="ignore", invalid="ignore"):
        m21 = np.where(l2 > 0, np.abs(l1 - g21 * l2) / l2, 0.0)
        m32 = np.where(l1 > 0, np.abs(l0 - g32 * l1) / l1, 0.0)
    sal = np.where(gate, np.maximum(l0.astype(np.float32), np.float32(0)), np.float32(0)).astype(np.float32)
    return {"count": count, "lam": lam, "gate": gate, "saliency": sal, "margin": np.minimum(m21, m32)}


def nms(saliency_, cloud, non_max_radius, min_neighbours, dist_mode, block=256, only=None):
    """bool [n] (or [len(only)]): the keypoints among the points of `cloud` with the float32 saliencies `saliency_` [n]."""
    cloud = np.ascontiguousarray(cloud, np.float32)
    s = np.ascontiguousarray(saliency_, np.float32)
    assert s.shape == (len(cloud),)
    own = np.arange(len(cloud)) if only is None else np.asarray(only, np.int64)
    index = np.arange(len(cloud))
    out = np.empty(len(own), bool)
    for lo in range(0, len(own), block):
        inside = _balls(cloud, non_max_radius, dist_mode, own, lo, block)
        rows = own[lo:lo + inside.shape[0]]
        mine = s[rows][:, None]
        dominates = (s[None, :] > mine) | ((s[None, :] == mine) & (index[None, :] < rows[:, None]))
        out[lo:lo + len(rows)] = (s[rows] > 0) & (inside.sum(axis=1) >= min_neighbours) & ~(inside & dominates).any(axis=1)
    return out


def keypoints(cloud, salient_radius, non_max_radius, dist_mode, gamma_21=0.975, gamma_32=0.975, min_neighbours=5):
    """(the saliency dict, keypoint bool [n]) of the whole restatement"""
    ref = saliency(cloud, salient_radius, dist_mode, gamma_21, gamma_32, min_neighbours)
    return ref, nms(ref["saliency"], cloud, non_max_radius, min_neighbours, dist_mode)
