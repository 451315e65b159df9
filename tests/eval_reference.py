"""The restatement mi_evaluate_registration is tested against (numpy, CPU): the rules of include/mi_slam.h retraced one by one.  The moving
cloud is moved in float32 numpy in the stated order (plane_reference.move_f32); the pair is the k = 1 answer of tests/knn_reference.py, or
the given index with knn_reference.d2_pairs' distance; the terms are float64, formed from the three rows of G = [-[a]x | I] with their
constants 0 and 1 in place, exactly as the header writes them.

Matrices here are indexed [row, col]; the C interface's column-major 4 x 4 is capi's business."""
import numpy as np

import knn_reference as K
import plane_reference as P


def rows_of_G(a):
    """the three rows of G = [-[a]x | I] for fixed points a float64 [p, 3]: three arrays [p, 6]"""
    ax, ay, az = a[:, 0], a[:, 1], a[:, 2]
    o, l = np.zeros(len(a)), np.ones(len(a))
    return (np.stack([o, az, -ay, l, o, o], axis=1), np.stack([-az, o, ax, o, l, o], axis=1), np.stack([ay, -ax, o, o, o, l], axis=1))


def sums_of_pairs(q, after, idx, d2):
    """(sums float64 [32], the sums of the terms' magnitudes) of the pairs (i, idx[i]) with idx[i] >= 0: the float64 terms of mi_slam.h, the
    moved points q and the pairs' float32 distances d2 being given"""
    after = np.ascontiguousarray(after, np.float32)
    pair = np.asarray(idx) >= 0
    jj = np.asarray(idx)[pair]
    a = after[jj].astype(np.float64)
    d = q[pair].astype(np.float64) - a
    G0, G1, G2 = rows_of_G(a)
    terms = [(G0[:, i] * G0[:, j] + G1[:, i] * G1[:, j]) + G2[:, i] * G2[:, j] for i in range(6) for j in range(i, 6)]
    terms += [(G0[:, i] * d[:, 0] + G1[:, i] * d[:, 1]) + G2[:, i] * d[:, 2] for i in range(6)]
    terms += [(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2], np.asarray(d2)[pair].astype(np.float64)]
    sums, mags = np.zeros(32), np.zeros(32)
    for k, term in enumerate(terms):
        sums[k], mags[k] = term.sum(), np.abs(term).sum()
    sums[29] = mags[29] = float(pair.sum())
    return sums, mags


def information(sums):
    """[6, 6]: the symmetric expansion of sums[0, 21); zeros with no pair"""
    return P.unpack_system(sums)[0] if sums[29] > 0 else np.zeros((6, 6))


def fitness_rmse(sums, n):
    """the two stated float64 expressions of a sums vector"""
    pairs = np.float64(sums[29])
    return pairs / np.float64(n), (np.sqrt(np.float64(sums[27]) / pairs) if pairs > 0 else np.float64(0))


def match(q, after, pairs=None, dist_mode=K.DIST_CPU_ROUNDING, max_d2=np.inf):
    """(idx int32 [n]: the fixed index of every pair or -1, d2 float32 [n]: its distance or +inf) of the moved points q"""
    after = np.ascontiguousarray(after, np.float32)
    n = len(q)
    if pairs is None:
        j, d2, count = K.unpack(K.sorted_keys(q, after, dist_mode, max_d2, keep=1), 1)
        j, d2 = j[:, 0], d2[:, 0]
        ok = (count == 1) & np.isfinite(d2)
    else:
        j = np.asarray(pairs, np.int32)
        assert j.shape == (n,) and ((j == -1) | ((j >= 0) & (j < len(after)))).all()
        has = j >= 0
        d2 = np.full(n, np.inf, np.float32)
        d2[has] = K.d2_pairs(q[has], after[j[has]], dist_mode)
        with np.errstate(invalid="ignore"):
            ok = has & (d2 <= np.float32(max_d2)) & np.isfinite(d2)
    return np.where(ok, j, -1).astype(np.int32), np.where(ok, d2, np.float32(np.inf)).astype(np.float32)


def evaluate(before, after, R=None, t=None, pairs=None, dist_mode=K.DIST_CPU_ROUNDING, max_d2=np.inf):
    """The whole call at the pose (R, t) (None: the identity) -> dict(fitness, rmse float64, sums float64 [32], abs float64 [32]: the sums
    of the terms' magnitudes, information float64 [6, 6], idx int32 [n], d2 float32 [n], q float32 [n, 3])."""
    R = np.eye(3) if R is None else R
    t = np.zeros(3) if t is None else t
    q = P.move_f32(R, t, before)
    idx, d2 = match(q, after, pairs, dist_mode, max_d2)
    sums, mags = sums_of_pairs(q, after, idx, d2)
    fitness, rmse = fitness_rmse(sums, len(q))
    return dict(fitness=fitness, rmse=rmse, sums=sums, abs=mags, information=information(sums), idx=idx, d2=d2, q=q)
