"""The restatement mi_remove_outliers is tested against (numpy, CPU), built on tests/knn_reference.py: the neighbours of the statistical
method are the sorted keys of the self-mode search (sorted_keys / unpack), the counts of the radius method come from the whole matrix
of squared distances (d2_matrix).  Scores, statistics and masks are float64, as include/mi_slam.h states them:

  statistical  mu_i = (sum of sqrt(float64(d2)) over row i's filled slots, nearest first) / count_i, 0 where count_i = 0;
               mean = sum mu / n, stddev = sqrt(sum (mu - mean)^2 / n), threshold = mean + float64(float32(std_ratio)) * stddev;
               kept iff mu_i <= threshold
  radius       r2 = float32(radius) * float32(radius); count_i = #{j != i (by index): d2(i, j) <= r2}; kept iff count_i >= min_neighbours"""
import numpy as np

import knn_reference as K


def scores(keys, k):
    """(mu float64 [n], count int32 [n]) from the self-mode sorted keys of a cloud (K.sorted_keys(None, cloud, mode))."""
    idx, d2, count = K.unpack(keys, k)
    roots = np.sqrt(d2.astype(np.float64))
    roots[idx == -1] = 0.0
    total = np.zeros(len(keys), np.float64)
    for r in range(k):                                  # nearest first, one addition per neighbour
        total = total + roots[:, r]
    mu = np.where(count > 0, total / np.maximum(count, 1), 0.0)
    return mu, count


def statistics(mu, std_ratio):
    """(mean, stddev, threshold) of the scores, float64."""
    n = len(mu)
    mean = mu.sum() / n
    stddev = np.sqrt(((mu - mean) ** 2).sum() / n)
    return float(mean), float(stddev), float(mean + np.float64(np.float32(std_ratio)) * stddev)


def statistical(cloud, k, dist_mode, std_ratio, keys=None):
    """(mu, count, (mean, stddev, threshold), keep bool [n])"""
    if keys is None:
        keys = K.sorted_keys(None, cloud, dist_mode)
    mu, count = scores(keys, k)
    st = statistics(mu, std_ratio)
    return mu, count, st, mu <= st[2]


def radius_counts(cloud, radius, dist_mode, block=256, only=None):
    """int32 [n]: the points j != i (by index) with d2(i, j) <= float32(radius)^2 in the arithmetic of dist_mode.
    only: the counts of the points `only` alone, [len(only)] -- what a large case can afford."""
    cloud = np.ascontiguousarray(cloud, np.float32)
    r2 = np.float32(radius) * np.float32(radius)
    own = np.arange(len(cloud)) if only is None else np.asarray(only, np.int64)
    out = np.empty(len(own), np.int32)
    for lo in range(0, len(own), block):
        inside = K.d2_matrix(cloud[own[lo:lo + block]], cloud, dist_mode) <= r2
        rows = inside.shape[0]
        inside[np.arange(rows), own[lo:lo + rows]] = False
        out[lo:lo + rows] = inside.sum(axis=1)
    return out


def radius(cloud, radius_, min_neighbours, dist_mode):
    """(count, keep bool [n])"""
    count = radius_counts(cloud, radius_, dist_mode)
    return count, count >= min_neighbours
