"""CPU suite: the float64 restatement of mi_fpfh_features (tests/fpfh_reference.py) against a plain scalar Python loop written from the
contract of include/mi_slam.h on its own, and against cases worked by hand."""
import math

import numpy as np
import pytest

import fpfh_reference as F
import knn_reference as K

MODES = (K.DIST_CPU_ROUNDING, K.DIST_FMA)


def unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


# ---- the contract once more, one pair and one point at a time, in Python floats
def scalar_pair(pi, ni, pj, nj):
    d = [pj[0] - pi[0], pj[1] - pi[1], pj[2] - pi[2]]
    length = math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    if length == 0:
        return 0.0, 0.0, 0.0
    a1 = ((ni[0] * d[0] + ni[1] * d[1]) + ni[2] * d[2]) / length
    a2 = ((nj[0] * d[0] + nj[1] * d[1]) + nj[2] * d[2]) / length
    if abs(a1) < abs(a2):
        u, t, d, phi = nj, ni, [-d[0], -d[1], -d[2]], -a2
    else:
        u, t, phi = ni, nj, a1
    v = [d[1] * u[2] - d[2] * u[1], d[2] * u[0] - d[0] * u[2], d[0] * u[1] - d[1] * u[0]]
    vl = math.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
    if vl == 0:
        return 0.0, 0.0, 0.0
    v = [v[0] / vl, v[1] / vl, v[2] / vl]
    w = [u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]]
    alpha = (v[0] * t[0] + v[1] * t[1]) + v[2] * t[2]
    theta = math.atan2((w[0] * t[0] + w[1] * t[1]) + w[2] * t[2], (u[0] * t[0] + u[1] * t[1]) + u[2] * t[2])
    return theta, alpha, phi


def scalar_bins(theta, alpha, phi):
    clamp = lambda x: 0 if math.isnan(x) else int(min(max(math.floor(x), 0), 10))
    pi = 3.141592653589793
    return clamp(11 * (theta + pi) / (2 * pi)), clamp(11 * (alpha + 1) * 0.5) + 11, clamp(11 * (phi + 1) * 0.5) + 22


def scalar_fpfh(cloud, normals, idx, d2):
    p = [[float(x) for x in row] for row in cloud]
    nr = [[float(x) for x in row] for row in normals]
    n, k = idx.shape
    counts = [[0] * 33 for _ in range(n)]
    count = [0] * n
    for i in range(n):
        for r in range(k):
            j = int(idx[i, r])
            if j < 0:
                continue
            count[i] += 1
            for b in scalar_bins(*scalar_pair(p[i], nr[i], p[j], nr[j])):
                counts[i][b] += 1
    s = [[(100.0 * c) / count[i] if count[i] else 0.0 for c in counts[i]] for i in range(n)]
    out = np.zeros((n, 33))
    for i in range(n):
        Fs, S = [0.0] * 33, [0.0] * 3
        for r in range(count[i]):
            j, w = int(idx[i, r]), float(d2[i, r])
            if not w > 0:
                continue
            for b in range(33):
                val = s[j][b] / w
                Fs[b] += val
                S[b // 11] += val
        scale = [100.0 / x if x != 0 else 0.0 for x in S]
        for b in range(33):
            out[i, b] = Fs[b] * scale[b // 11] + s[i][b]
    return out, np.array(counts), np.array(count)


@pytest.mark.parametrize("mode", MODES)
def test_the_restatement_against_a_scalar_loop(mode):
    rng = np.random.default_rng(181 + mode)
    n, k = 60, 5
    cloud = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    cloud[7] = cloud[3]                                             # a duplicate
    normals = unit(rng.normal(size=(n, 3))).astype(np.float32)
    normals[11] = 0                                                 # a zero normal
    idx, d2, count = K.knn(None, cloud, k, mode)
    fpfh, counts, count_ref, fragile = F.from_neighbours(cloud, normals, idx, d2)
    want, want_counts, want_count = scalar_fpfh(cloud, normals, idx, d2)
    # (the zero normal makes theta an atan2 of signed zeros, 0 or +-pi: an edge, so its pairs are fragile -- and still equal here)
    touches = (idx == 11).any(axis=1) | (np.arange(n) == 11)
    assert not fragile[~(touches | touches[idx].any(axis=1))].any()
    assert np.array_equal(count_ref, count) and np.array_equal(want_count, count)
    assert np.array_equal(counts, want_counts)
    # numpy's atan2 and Python's may differ in the last bit, which no bin away from an edge sees; the sums then are the same operations
    assert np.array_equal(fpfh, want)
    again = F.fpfh(cloud, normals, k, mode)
    assert np.array_equal(again[0], fpfh) and np.array_equal(again[1], counts)
    # pair by pair
    i = np.repeat(np.arange(n), k)
    j = idx.reshape(-1)
    feats = F.pair_features(cloud[i], normals[i], cloud[j], normals[j])
    bins = F.bins(feats)
    for row in range(n * k):
        f = scalar_pair(*[[float(x) for x in a] for a in (cloud[i[row]], normals[i[row]], cloud[j[row]], normals[j[row]])])
        assert np.allclose(feats[row], f, rtol=0, atol=1e-15), row
        assert tuple(bins[row]) == scalar_bins(*f), row


def test_bins_at_the_ends_and_nan():
    f = np.array([[-np.pi, -1.0, -1.0], [np.pi, 1.0, 1.0], [0.0, 0.0, 0.0], [np.nan, np.nan, np.nan], [4.0, 1.5, -1.5]])
    assert F.bins(f).tolist() == [[0, 11, 22], [10, 21, 32], [5, 16, 27], [0, 11, 22], [10, 21, 22]]
    # an interior edge of alpha: 11 (alpha + 1) / 2 = 3 at alpha = -5 / 11
    edge = np.array([[0.1, -5.0 / 11.0, 0.3]])
    assert F.near_an_edge(edge).all() and not F.near_an_edge(edge + 1e-6).any()
    assert F.near_an_edge(np.array([[np.pi, 0.0, 0.0], [-np.pi, 0.0, 0.0]])).all()        # +-pi is an edge for theta ...
    assert not F.near_an_edge(np.array([[0.0, 1.0, -1.0]])).any()                          # ... the clamped ends of alpha and phi are none


def test_a_planar_lattice_has_one_bin_per_feature():
    g = np.arange(5, dtype=np.float32)
    cloud = np.stack([np.repeat(g, 5), np.tile(g, 5), np.zeros(25, np.float32)], axis=1)
    normals = np.tile(np.array([[0, 0, 1]], np.float32), (25, 1))
    for k in (4, 8):
        fpfh, counts, count, fragile = F.fpfh(cloud, normals, k)
        assert (count == k).all() and not fragile.any()
        want = np.zeros((25, 33), np.int64)
        want[:, [5, 16, 27]] = k
        assert np.array_equal(counts, want)
        assert np.array_equal(fpfh, np.where(want > 0, 200.0, 0.0))


def test_two_points_by_hand():
    """p0 = (0, 0, 0), n0 = (0, 0, 1); p1 = (1, 0, 0), n1 = (0.6, 0, 0.8).  Pair (0, 1): d = (1, 0, 0), a1 = 0, a2 = 0.6, so the roles swap:
    u = n1, t = n0, d = (-1, 0, 0), phi = -0.6; v = d x u = (0, 0.8, 0) -> (0, 1, 0); w = u x v = (-0.8, 0, 0.6); alpha = 0;
    theta = atan2(0.6, 0.8).  Pair (1, 0): d = (-1, 0, 0), a1 = n1 . d = -0.6, a2 = 0: no swap, the same frame and the same features.
    Bins: theta 11 (0.6435 + pi) / (2 pi) = 6.63 -> 6; alpha 5.5 -> 5 (+ 11); phi 11 x 0.4 / 2 = 2.2 -> 2 (+ 22).  Each point has the
    other at d2 = 1: F = s = 100 in those bins, S = 100, scale = 1, fpfh = 100 + 100."""
    cloud = np.array([[0, 0, 0], [1, 0, 0]], np.float32)
    normals = np.array([[0, 0, 1], [0.6, 0, 0.8]], np.float32)
    feats, fragile = F.pair_features_and_fragility(cloud[[0, 1]], normals[[0, 1]], cloud[[1, 0]], normals[[1, 0]])
    assert not fragile.any()
    assert np.allclose(feats, [[math.atan2(0.6, 0.8), 0.0, -0.6]] * 2, rtol=0, atol=1e-7)      # (0.6 and 0.8 are rounded to fp32)
    assert np.array_equal(feats[0], feats[1])
    assert F.bins(feats).tolist() == [[6, 16, 24]] * 2
    fpfh, counts, count, fragile = F.fpfh(cloud, normals, 3)
    assert count.tolist() == [1, 1] and not fragile.any()
    want = np.zeros((2, 33))
    want[:, [6, 16, 24]] = 1
    assert np.array_equal(counts, want) and np.array_equal(fpfh, 200.0 * want)


def test_duplicates_count_as_pairs_and_not_as_weights():
    cloud = np.array([[0.5, 0.25, 0], [0.5, 0.25, 0], [1.5, 0.5, 0.25]], np.float32)
    normals = unit([[0, 0.2, 1], [0.3, 0, 1], [0.1, 0.1, 1]]).astype(np.float32)
    fpfh, counts, count, fragile = F.fpfh(cloud, normals, 2)
    assert count.tolist() == [2, 2, 2] and not fragile.any()
    for i in (0, 1):                                     # the twin at len 0 is in bins 5 / 16 / 27 ...
        assert (counts[i, [5, 16, 27]] >= 1).all()
    s = 100.0 * counts / 2.0
    for i in (0, 1):                                     # ... and only the third point weighs: F / S x 100 is its SPFH again
        assert np.allclose(fpfh[i], s[2] + s[i], rtol=1e-14, atol=0)
    assert np.allclose(fpfh.reshape(3, 3, 11).sum(axis=2), 200.0, rtol=1e-14)
    # a cloud of twins alone: every pair is degenerate, nothing weighs, and the descriptor is the point's own SPFH
    fpfh, counts, count, _ = F.fpfh(cloud[[0, 0, 0]], normals, 2)
    want = np.zeros((3, 33))
    want[:, [5, 16, 27]] = 2
    assert np.array_equal(counts, want) and np.array_equal(fpfh, 50.0 * want)


def test_a_point_alone_within_the_limit_gets_zeros():
    cloud = np.array([[0, 0, 0], [0.1, 0, 0], [0, 0.1, 0], [50, 50, 50]], np.float32)
    normals = unit([[0, 0.1, 1], [0.2, 0, 1], [0, 0, 1], [1, 1, 1]]).astype(np.float32)
    fpfh, counts, count, _ = F.fpfh(cloud, normals, 3, max_d2=1.0)
    assert count.tolist() == [2, 2, 2, 0]
    assert (fpfh[3] == 0).all() and (counts[3] == 0).all()
    assert np.allclose(fpfh[:3].reshape(3, 3, 11).sum(axis=2), 200.0, rtol=1e-14)


@pytest.mark.parametrize("mode", MODES)
def test_block_sums_on_a_random_cloud(mode):
    rng = np.random.default_rng(191)
    n, k = 500, 10
    cloud = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    normals = unit(rng.normal(size=(n, 3))).astype(np.float32)
    fpfh, counts, count, fragile = F.fpfh(cloud, normals, k, mode)
    assert (count == k).all() and fragile.sum() <= 0.001 * n
    assert (counts.reshape(n, 3, 11).sum(axis=2) == k).all()
    assert (fpfh >= 0).all() and np.allclose(fpfh.reshape(n, 3, 11).sum(axis=2), 200.0, rtol=1e-13)
    assert len(np.unique(counts.argmax(axis=1))) > 1       # the descriptor tells points apart
