"""The restatement mi_fpfh_features is tested against (numpy, CPU, float64), following the contract of include/mi_slam.h operation for
operation: the Darboux-frame features of every (point, neighbour) pair, their bins, the SPFH counts, and the distance-weighted sums of
the neighbours' SPFH in key order.  The neighbour lists come in from outside (tests/knn_reference.py in self mode, or the device's own
mi_knn_search, which is tested on its own), like those of tests/normals_reference.py.

Fragile pairs.  The bins and the swap of the frame are discontinuous, and atan2 may differ in its last bit between numpy and the device.
A pair is fragile when
  - a feature lies within EDGE = 1e-9 bin widths of an interior bin edge (for theta, +-pi counts as an edge too),
  - | |a1| - |a2| | <= 1e-9 without both being exactly 0,
  - 0 < vl < 1e-6 len |u|,
  - hypot(w . t, u . t) < 1e-6 |t| with t nonzero.
A point is fragile when a pair of its own row is, or a pair of any of its neighbours' rows is: its counts, or the SPFH it gathers, may
then differ by one pair."""
import numpy as np

import knn_reference as K

BINS, DIM = 11, 33
PI = 3.141592653589793
EDGE = 1e-9


def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


def pair_features_and_fragility(p_i, n_i, p_j, n_j):
    """(features float64 [m, 3]: theta, alpha, phi; fragile bool [m]) of m pairs; the bins' own edges are not looked at here"""
    p_i, n_i, p_j, n_j = (np.asarray(a, np.float64).reshape(-1, 3) for a in (p_i, n_i, p_j, n_j))
    m = len(p_i)
    out = np.zeros((m, 3))
    fragile = np.zeros(m, bool)
    with np.errstate(all="ignore"):
        d = p_j - p_i
        length = np.sqrt(_dot(d, d))
        live = length != 0
        a1 = _dot(n_i, d) / length
        a2 = _dot(n_j, d) / length
        swap = np.abs(a1) < np.abs(a2)
        tie = np.abs(np.abs(a1) - np.abs(a2)) <= 1e-9
        fragile |= live & tie & ~((a1 == 0) & (a2 == 0))
        u = np.where(swap[:, None], n_j, n_i)
        t = np.where(swap[:, None], n_i, n_j)
        d = np.where(swap[:, None], -d, d)
        phi = np.where(swap, -a2, a1)
        v = _cross(d, u)
        vl = np.sqrt(_dot(v, v))
        fragile |= live & (vl > 0) & (vl < 1e-6 * length * np.sqrt(_dot(u, u)))
        live &= vl != 0
        v = v / vl[:, None]
        w = _cross(u, v)
        alpha = _dot(v, t)
        y, x = _dot(w, t), _dot(u, t)
        theta = np.arctan2(y, x)
        tl = np.sqrt(_dot(t, t))
        fragile |= live & (tl > 0) & (np.hypot(y, x) < 1e-6 * tl)
    out[live, 0], out[live, 1], out[live, 2] = theta[live], alpha[live], phi[live]
    return out, fragile


def pair_features(p_i, n_i, p_j, n_j):
    return pair_features_and_fragility(p_i, n_i, p_j, n_j)[0]


def _scaled(features):
    """every feature in units of its bins: [m, 3], bin b is [b, b + 1)"""
    f = np.asarray(features, np.float64).reshape(-1, 3)
    return np.stack([(11.0 * (f[:, 0] + PI)) / (2.0 * PI), (11.0 * (f[:, 1] + 1.0)) * 0.5, (11.0 * (f[:, 2] + 1.0)) * 0.5], axis=1)


def bins(features):
    """int64 [m, 3]: the bins of theta, alpha, phi in the descriptor's 33 (theta's in [0, 11), alpha's in [11, 22), phi's in [22, 33))"""
    x = _scaled(features)
    with np.errstate(invalid="ignore"):
        b = np.where(np.isnan(x), 0.0, np.clip(np.floor(x), 0.0, 10.0)).astype(np.int64)
    return b + np.array([0, BINS, 2 * BINS])


def near_an_edge(features):
    """bool [m]: a feature within EDGE bin widths of an interior bin edge, or theta within that of +-pi"""
    x = _scaled(features)
    nearest = np.round(x)
    close = np.abs(x - nearest) <= EDGE
    interior = (nearest >= 1) & (nearest <= 10)
    ends = (nearest == 0) | (nearest == 11)
    return (close & interior).any(axis=1) | (close[:, 0] & ends[:, 0])


def from_neighbours(cloud, normals, idx, d2):
    """(fpfh float64 [n, 33], counts int64 [n, 33], count int32 [n], fragile bool [n]) from the neighbour lists idx [n, k] (-1: no
    neighbour in that slot) and their float32 squared distances d2 [n, k], both in key order."""
    p = np.ascontiguousarray(cloud, np.float32).astype(np.float64)
    nrm = np.ascontiguousarray(normals, np.float32).astype(np.float64)
    idx = np.asarray(idx)
    n, k = idx.shape
    have = idx >= 0
    j = np.where(have, idx, 0).astype(np.int64)
    count = have.sum(axis=1).astype(np.int32)
    i = np.repeat(np.arange(n), k)
    jf = j.reshape(-1)
    feats, frag = pair_features_and_fragility(p[i], nrm[i], p[jf], nrm[jf])
    frag |= near_an_edge(feats)
    b = bins(feats)                                                                   # [n k, 3]
    counts = np.zeros(n * DIM, np.int64)
    for f in range(3):
        counts += np.bincount(i * DIM + b[:, f], weights=have.reshape(-1).astype(np.float64), minlength=n * DIM).astype(np.int64)
    counts = counts.reshape(n, DIM)
    assert (counts.reshape(n, 3, BINS).sum(axis=2) == count[:, None]).all()
    with np.errstate(all="ignore"):
        s = np.where(count[:, None] > 0, (100.0 * counts) / count[:, None].astype(np.float64), 0.0)
    F, S = np.zeros((n, DIM)), np.zeros((n, 3))
    d2 = np.asarray(d2, np.float32).astype(np.float64)
    for r in range(k):
        use = have[:, r] & (d2[:, r] > 0)
        with np.errstate(all="ignore"):
            val = np.where(use[:, None], s[j[:, r]] / d2[:, r][:, None], 0.0)            # (+ 0.0 leaves a sum's bits alone)
        F += val
        for c in range(DIM):
            S[:, c // BINS] += val[:, c]
    with np.errstate(all="ignore"):
        scale = np.where(S != 0, 100.0 / S, 0.0)
    fpfh = F * np.repeat(scale, BINS, axis=1) + s
    own = (frag.reshape(n, k) & have).any(axis=1)
    fragile = own | (own[j] & have).any(axis=1)
    return fpfh, counts, count, fragile


def fpfh(cloud, normals, k, dist_mode=K.DIST_CPU_ROUNDING, max_d2=np.inf):
    idx, d2, _ = K.knn(None, cloud, k, dist_mode, max_d2)
    return from_neighbours(cloud, normals, idx, d2)


# ---- what a test compares (bounds: none is taken from the device)
REL = 2.0 ** -23           # one fp32 rounding, 2^-24, doubled; the fp64 chain of at most 32 x 2 operations adds about 1e-14


def check(ref, got, what, max_fragile_share=0.001):
    """fpfh float32 [n, 33], counts [n, 33], count [n] of the device against from_neighbours' answer.  Non-fragile points: counts equal,
    |fpfh - ref| <= 2^-23 |ref|, exactly 0 where ref is.  Every point: count equal, each block of counts sums to count, each block of fpfh
    sums to 200 within 2^-23 x 200 (100 where every neighbour is a duplicate, 0 without neighbours).  At most max_fragile_share of the points
    may be fragile."""
    fpfh_ref, counts_ref, count_ref, fragile = ref
    fpfh_got, counts_got, count_got = got
    n = len(count_ref)
    assert fpfh_got.shape == (n, DIM) and fpfh_got.dtype == np.float32 and np.isfinite(fpfh_got).all(), what
    assert np.array_equal(count_got, count_ref), what
    assert fragile.sum() <= max_fragile_share * n, (what, int(fragile.sum()), n)
    ok = ~fragile
    assert np.array_equal(counts_got.astype(np.int64).reshape(n, 3, BINS).sum(axis=2), np.repeat(count_ref[:, None], 3, axis=1)), what
    assert np.array_equal(counts_got[ok].astype(np.int64), counts_ref[ok]), what
    g = fpfh_got.astype(np.float64)
    err = np.abs(g - fpfh_ref)[ok]
    mag = np.abs(fpfh_ref)[ok]
    worst = (err[mag > 0] / mag[mag > 0]).max(initial=0.0)
    print("%s: %d points, %d fragile; fpfh relative error %.3e (bound %.3e)" % (what, n, int(fragile.sum()), worst, REL))
    assert (err <= REL * mag).all(), (what, worst)
    assert (g[ok][mag == 0] == 0).all(), what
    want = np.round(fpfh_ref.reshape(n, 3, BINS).sum(axis=2) / 100.0) * 100.0            # 200, 100 or 0: the reference's own sums, to the integer they are
    assert np.isin(want, (0.0, 100.0, 200.0)).all(), what
    sums = g.reshape(n, 3, BINS).sum(axis=2)
    assert (np.abs(sums - want) <= REL * 200.0).all(), (what, np.abs(sums - want).max())
