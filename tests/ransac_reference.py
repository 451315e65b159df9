"""The contract of mi_ransac_register (include/mi_slam.h) restated in numpy: the counter-based draws in exact integer arithmetic, the edge
rule and the count rule in float64 in the header's order of operations, and a float64 Kabsch of the three pairs (numpy's SVD) beside
the device's fp32 one.  What float64 cannot decide is marked fragile rather than decided."""
import numpy as np

from kabsch_catalogue import kabsch64

MASK = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
FRAGILE = 1e-12                                       # relative distance to a threshold below which float64 orders do not bind the device
COLLINEAR = 1e-5                                      # sigma_2 / sigma_1 of H below which the fp32 SVD's sigma_2 > 0 test is not predicted


def mix(z):
    """the splitmix64 finaliser on a python int"""
    z &= MASK
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & MASK
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def draws(seed, h, C):
    """the three ranks of hypothesis h"""
    return [(((mix(seed + GOLDEN * (3 * h + r + 1)) >> 32) * C) >> 32) for r in range(3)]


def ranks(seed, first, count, C):
    """int64 [count, 3], vectorised (uint64 arithmetic wraps modulo 2^64 as the contract's does)"""
    with np.errstate(over="ignore"):
        h = np.arange(first, first + count, dtype=np.uint64)[:, None]
        z = np.uint64(seed & MASK) + np.uint64(GOLDEN) * (np.uint64(3) * h + np.arange(1, 4, dtype=np.uint64)[None, :])
        z ^= z >> np.uint64(30)
        z *= np.uint64(0xBF58476D1CE4E5B9)
        z ^= z >> np.uint64(27)
        z *= np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
        return (((z >> np.uint64(32)) * np.uint64(C)) >> np.uint64(32)).astype(np.int64)


def correspondences(src, tgt, idx):
    """(source index per rank, s [C, 3] float64, t [C, 3] float64)"""
    i = np.flatnonzero(np.asarray(idx) >= 0)
    return i, np.asarray(src, np.float32)[i].astype(np.float64), np.asarray(tgt, np.float32)[np.asarray(idx)[i]].astype(np.float64)


def len2(d):
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def edge_rule(s3, t3, edge_similarity):
    """s3, t3 [H, 3, 3] (hypothesis, draw, xyz): (valid, fragile) -- fragile where a ratio is within FRAGILE of the threshold"""
    e2 = float(np.float32(edge_similarity)) * float(np.float32(edge_similarity))
    ok, fragile = np.ones(len(s3), bool), np.zeros(len(s3), bool)
    for p, q in ((0, 1), (1, 2), (0, 2)):
        ls2, lt2 = len2(s3[:, p] - s3[:, q]), len2(t3[:, p] - t3[:, q])
        for a, b in ((ls2, e2 * lt2), (lt2, e2 * ls2)):
            ok &= a >= b
            fragile |= (np.abs(a - b) <= FRAGILE * np.maximum(a, b)) & (e2 > 0)
    return ok, fragile


def cross_covariance(s3, t3):
    """(H float32-rounded as float64 [H, 3, 3], cb, ca): the header's moments"""
    cb, ca = ((s3[:, 0] + s3[:, 1]) + s3[:, 2]) * (1.0 / 3.0), ((t3[:, 0] + t3[:, 1]) + t3[:, 2]) * (1.0 / 3.0)
    m = (t3[:, 0, :, None] * s3[:, 0, None, :] + t3[:, 1, :, None] * s3[:, 1, None, :]) + t3[:, 2, :, None] * s3[:, 2, None, :]
    return (m - 3.0 * ca[:, :, None] * cb[:, None, :]).astype(np.float32).astype(np.float64), cb, ca


def hypotheses(src, tgt, idx, seed, first, count, edge_similarity):
    """dict: triples [count, 3] (source indices), valid, fragile, H (fp32-rounded), cb, ca, R64, t64, S64, d, g"""
    i, s, t = correspondences(src, tgt, idx)
    rk = ranks(seed, first, count, len(i))
    s3, t3 = s[rk], t[rk]
    distinct = (rk[:, 0] != rk[:, 1]) & (rk[:, 0] != rk[:, 2]) & (rk[:, 1] != rk[:, 2])
    ok, fragile = edge_rule(s3, t3, edge_similarity)
    H, cb, ca = cross_covariance(s3, t3)
    R64, S, d, g = kabsch64(H)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(S[:, 0] > 0, S[:, 1] / np.where(S[:, 0] > 0, S[:, 0], 1.0), 0.0)
    collinear = ratio == 0
    fragile = distinct & (fragile | (ok & ~collinear & (ratio < COLLINEAR)))
    t64 = ca - np.einsum("nij,nj->ni", R64, cb)
    return dict(triples=i[rk], valid=distinct & ok & ~collinear, fragile=fragile, H=H, cb=cb, ca=ca, R64=R64, t64=t64, S=S, d=d, g=g)


def count_rule(pose12, s, t, max_distance):
    """float64 recount under fp32 poses [K, 12] (R9 column-major, t3): (lowest, highest possible inlier count per pose) -- they differ
    where a pair's squared distance is within FRAGILE of the threshold; and the d2 matrix [K, C]"""
    P = np.asarray(pose12, np.float32).astype(np.float64)
    md2 = float(np.float32(max_distance)) * float(np.float32(max_distance))
    d = []
    for r in range(3):
        p = ((P[:, None, r] * s[None, :, 0] + P[:, None, 3 + r] * s[None, :, 1]) + P[:, None, 6 + r] * s[None, :, 2]) + P[:, None, 9 + r]
        d.append(p - t[None, :, r])
    d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
    near = np.abs(d2 - md2) <= FRAGILE * md2
    inl = d2 <= md2
    return (inl & ~near).sum(axis=1), (inl | near).sum(axis=1), d2


def kabsch_pairs64(s, t):
    """float64 Kabsch of pairs s -> t: (R, t)"""
    cb, ca = s.mean(axis=0), t.mean(axis=0)
    R, S, d, g = kabsch64(((t - ca).T @ (s - cb))[None])
    return R[0], ca - R[0] @ cb


def planted(seed=2026, n=2000):
    """The planted problem of the GPU suite: 2 000 source points uniform in a cube, target = R0 source + t0 + 1e-3 noise with a rotation of
    100 degrees; idx true for 30 % of the points, uniformly random for 60 %, -1 for 10 %.  (src, tgt, idx, R0, t0, true mask)
    n: the same recipe with another number of points (a multiple of 10)."""
    rng = np.random.default_rng(seed)
    a30, a90 = 3 * n // 10, 9 * n // 10
    src = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    axis = np.array([0.3, -0.5, 0.8])
    axis /= np.linalg.norm(axis)
    a = np.deg2rad(100.0)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    R0 = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K
    t0 = np.array([0.5, -1.0, 2.0])
    tgt = (src.astype(np.float64) @ R0.T + t0 + 1e-3 * rng.uniform(-1, 1, (n, 3)) / np.sqrt(3)).astype(np.float32)
    kind = rng.permutation(n)
    idx = np.arange(n, dtype=np.int32)
    idx[kind[a30:a90]] = rng.integers(0, n, a90 - a30)
    idx[kind[a90:]] = -1
    true = np.zeros(n, bool)
    true[kind[:a30]] = True
    return src, tgt, idx, R0, t0, true
