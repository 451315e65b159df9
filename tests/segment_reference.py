"""The contract of mi_segment_plane (include/mi_slam.h) restated in numpy: the counter-based draws in exact integer arithmetic with the
global hypothesis number, the plane through three points in float64 in the header's order of operations and rounded to float32, the axis
rule, the count rule, the winner, the refinement (the fixed-order sums, numpy.linalg.eigh beside the device's Jacobi sweeps), rmse and the
peel.  Everything is float64 arithmetic on float32 values, one operation at a time: numpy never fuses."""
import numpy as np

from ransac_reference import ranks

BLOCK = 256


def planes_through(p, axis=None, min_axis_cosine=0.0):
    """The planes through triples p [K, draw, xyz] (float32 values): (valid [K] bool, plane4 [K, 4] float32, zeros where invalid)"""
    p = np.asarray(p, np.float32).astype(np.float64)
    e1, e2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    with np.errstate(all="ignore"):
        Nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        Ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        Nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        len2 = (Nx * Nx + Ny * Ny) + Nz * Nz
        valid = (len2 > 0) & np.isfinite(len2)
        q = 1.0 / np.sqrt(np.where(valid, len2, 1.0))
        plane = np.stack([Nx * q, Ny * q, Nz * q, -(((Nx * p[:, 0, 0] + Ny * p[:, 0, 1]) + Nz * p[:, 0, 2]) * q)], axis=1).astype(np.float32)
        valid &= np.isfinite(plane).all(axis=1)
        if axis is not None:
            ax = np.asarray(axis, np.float32).astype(np.float64)
            cos = float(np.float32(min_axis_cosine))
            P = plane.astype(np.float64)
            dot = (P[:, 0] * ax[0] + P[:, 1] * ax[1]) + P[:, 2] * ax[2]
            aa = (ax[0] * ax[0] + ax[1] * ax[1]) + ax[2] * ax[2]
            nn = (P[:, 0] * P[:, 0] + P[:, 1] * P[:, 1]) + P[:, 2] * P[:, 2]
            valid &= dot * dot >= (cos * cos) * (aa * nn)
    plane[~valid] = 0
    return valid, plane


def hypotheses(rem, index, seed, g0, count, axis=None, min_axis_cosine=0.0):
    """Hypotheses g0 .. g0 + count - 1 over the remaining points rem [C, 3] float32 with caller indices index [C]:
    (triples [count, 3], valid [count] bool, plane4 [count, 4] float32, zeros where invalid)"""
    rem = np.asarray(rem, np.float32)
    rk = ranks(seed, g0, count, len(rem))
    distinct = (rk[:, 0] != rk[:, 1]) & (rk[:, 0] != rk[:, 2]) & (rk[:, 1] != rk[:, 2])
    valid, plane = planes_through(rem[rk], axis, min_axis_cosine)
    plane[~distinct] = 0
    return np.asarray(index)[rk].astype(np.int32), valid & distinct, plane


def signed(plane4, rem):
    """float64 s [K, C] and nn [K] of fp32 planes [K, 4] over points rem [C, 3]: the count rule's terms"""
    P = np.atleast_2d(np.asarray(plane4, np.float32)).astype(np.float64)
    x = np.asarray(rem, np.float32).astype(np.float64)
    s = ((P[:, None, 0] * x[None, :, 0] + P[:, None, 1] * x[None, :, 1]) + P[:, None, 2] * x[None, :, 2]) + P[:, None, 3]
    return s, (P[:, 0] * P[:, 0] + P[:, 1] * P[:, 1]) + P[:, 2] * P[:, 2]


def inlier_mask(plane4, rem, thr):
    """bool [K, C]: s s <= T2 nn"""
    s, nn = signed(plane4, rem)
    T2 = float(np.float32(thr)) * float(np.float32(thr))
    return s * s <= (T2 * nn)[:, None]


def counts(plane4, valid, rem, thr, chunk=256):
    """inlier counts [K] under the count rule; 0 for invalid hypotheses"""
    plane4 = np.atleast_2d(plane4)
    out = np.zeros(len(plane4), np.int64)
    for lo in range(0, len(plane4), chunk):
        out[lo:lo + chunk] = inlier_mask(plane4[lo:lo + chunk], rem, thr).sum(axis=1)
    return np.where(valid, out, 0).astype(np.int32)


def fixed_sum(v):
    """the fixed order of every sum: rank r to partial sum r mod 256 in ascending r, the partial sums added pairwise at strides 128 .. 1.
    v [C] float64, zero where the point does not count (x + 0.0 is x)"""
    v = np.asarray(v, np.float64)
    rows = -(-len(v) // BLOCK)
    padded = np.zeros(rows * BLOCK)
    padded[:len(v)] = v
    acc = np.zeros(BLOCK)
    for row in padded.reshape(rows, BLOCK):
        acc = acc + row
    w = BLOCK // 2
    while w > 0:
        acc[:w] = acc[:w] + acc[w:2 * w]
        w //= 2
    return float(acc[0])


def scatter(rem, mask):
    """(count, centroid [3], the six sums xx xy xz yy yz zz about it) of the flagged points, every sum in the fixed order"""
    x = np.asarray(rem, np.float32).astype(np.float64)
    count = int(mask.sum())
    c = np.array([fixed_sum(np.where(mask, x[:, k], 0.0)) for k in range(3)]) / float(count)
    d = x - c
    six = [fixed_sum(np.where(mask, d[:, i] * d[:, j], 0.0)) for i, j in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))]
    return count, c, np.array(six)


def refit(rem, mask, prev):
    """the least-squares plane of the flagged points, turned towards prev [4] float32: float32 [4] (eigh instead of the device's sweeps)"""
    count, c, six = scatter(rem, mask)
    M = np.array([[six[0], six[1], six[2]], [six[1], six[3], six[4]], [six[2], six[4], six[5]]])
    n = np.linalg.eigh(M)[1][:, 0]
    pv = np.asarray(prev, np.float32).astype(np.float64)
    if (n[0] * pv[0] + n[1] * pv[1]) + n[2] * pv[2] < 0:
        n = -n
    d = -((n[0] * c[0] + n[1] * c[1]) + n[2] * c[2])
    return np.array([n[0], n[1], n[2], d]).astype(np.float32)


def rmse_of(plane, rem, mask, thr=None):
    """(float)sqrt(S / count), S the fixed-order sum of s s / nn over the flagged points"""
    s, nn = signed(plane, rem)
    S = fixed_sum(np.where(mask, (s[0] * s[0]) / nn[0], 0.0))
    return np.float32(np.sqrt(S / float(mask.sum())))


def segment(cloud, thr, hypotheses_per_plane=1000, seed=0, refine_iterations=2, max_planes=1, min_inliers=3, axis=None, min_axis_cosine=0.0):
    """The whole call: dict(planes [P, 4] float32, inliers [P], labels [n], rmse [P] float32, winners [P], n_planes)"""
    cloud = np.asarray(cloud, np.float32)
    n, H = len(cloud), int(hypotheses_per_plane)
    labels = np.full(n, -1, np.int32)
    planes, inliers, rmses, winners = [], [], [], []
    for p in range(max_planes):
        index = np.flatnonzero(labels < 0)
        C = len(index)
        if C < 3 or C < min_inliers:
            break
        rem = cloud[index]
        _, valid, plane4 = hypotheses(rem, index, seed, p * H, H, axis, min_axis_cosine)
        if not valid.any():
            break
        cnt = counts(plane4, valid, rem, thr)
        h = int(np.flatnonzero(valid)[np.argmax(cnt[valid])])        # argmax returns the first maximum: the lowest h among equals
        if cnt[h] < min_inliers:
            break
        plane, mask = plane4[h].copy(), inlier_mask(plane4[h], rem, thr)[0]
        for _ in range(refine_iterations):
            if mask.sum() < 3:
                break
            trial = refit(rem, mask, plane)
            if not np.isfinite(trial).all():
                break
            trial_mask = inlier_mask(trial, rem, thr)[0]
            if trial_mask.sum() < 3:
                break
            plane, mask = trial, trial_mask
        labels[index[mask]] = len(planes)
        planes.append(plane)
        inliers.append(int(mask.sum()))
        rmses.append(rmse_of(plane, rem, mask))
        winners.append(h)
    return dict(planes=np.array(planes, np.float32).reshape(-1, 4), inliers=np.array(inliers, np.int32), labels=labels,
                rmse=np.array(rmses, np.float32), winners=np.array(winners, np.int32), n_planes=len(planes))
