"""The contract of mi_feature_match (include/mi_slam.h) restated in numpy, with the fp32 fmaf emulated exactly.

fmaf(a, b, c) of three fp32 values: the product a * b of two 24-bit significands has at most 48 bits and is exact in float64 (for the
magnitudes the contract admits, |a|, |b| <= 1e15, and down to products of fp32 subnormals, it is far inside float64's exponent range).  The
sum p + c is taken in float64 together with its exact error term (TwoSum, Knuth).  Rounding the float64 sum to fp32 directly would round
twice; the error term settles it: where the sum is inexact and its last float64 bit is even, it is moved one float64 step towards the
exact value, which makes the last bit odd ("round to odd").  A value rounded to odd at 53 bits rounds to fp32 (24 bits, 29 fewer) exactly
as the unrounded value does: it can sit on a tie of the fp32 grid only if the exact sum does, and otherwise lies strictly on the exact
sum's side of it -- the error term breaks the tie."""
import numpy as np

MAX_DIM = 64
MAX_ABS = 1e15


def fmaf(a, b, c):
    """fp32 fma of float32 arrays (broadcast), one rounding: float32"""
    a, b, c = (np.asarray(v, np.float32).astype(np.float64) for v in (a, b, c))
    with np.errstate(over="ignore", invalid="ignore"):
        p = a * b                                    # exact
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)              # TwoSum: p + c = s + err exactly
        bits = np.ascontiguousarray(s).view(np.int64)
        fix = (err != 0) & np.isfinite(s) & ((bits & 1) == 0)
        away = (err > 0) == (s > 0)                  # the exact value lies farther from zero than s (s != 0 wherever err != 0)
        odd = (bits + np.where(away, 1, -1)).view(np.float64)
        return np.where(fix, odd, s).astype(np.float32)


def fmaf_scalar(a, b, c):
    """The same through exact rational arithmetic, one value at a time (the check of fmaf; finite operands)."""
    from fractions import Fraction
    x = Fraction(float(np.float32(a))) * Fraction(float(np.float32(b))) + Fraction(float(np.float32(c)))
    if x == 0:
        return np.float32(0.0)
    r = np.float32(float(x))                         # double rounding possible: repaired below
    lo, hi = np.nextafter(r, np.float32(-np.inf)), np.nextafter(r, np.float32(np.inf))
    best = min((v for v in (lo, r, hi) if np.isfinite(v)), key=lambda v: (abs(Fraction(float(v)) - x), int(np.float32(v).view(np.uint32)) & 1))
    return np.float32(best)                          # nearest; on a tie the even significand


def chain(q, t):
    """dot(i, j) of every pair: float32 [n, m].  q [n, dim], t [m, dim] float32."""
    q, t = np.asarray(q, np.float32), np.asarray(t, np.float32)
    c = np.zeros((q.shape[0], t.shape[0]), np.float32)
    for b in range(q.shape[1]):
        c = fmaf(q[:, b][:, None], t[:, b][None, :], c)
    return c


def norms(x):
    x = np.asarray(x, np.float32)
    c = np.zeros(x.shape[0], np.float32)
    for b in range(x.shape[1]):
        c = fmaf(x[:, b], x[:, b], c)
    return c


def keys(q, t):
    """(h [n, m], g [m, n]) float32: the forward and the reverse keys"""
    dot = chain(q, t)
    return fmaf(np.float32(-2.0), dot, norms(t)[None, :]), fmaf(np.float32(-2.0), dot.T, norms(q)[None, :])


def directions(q, t):
    """(forward int32 [n], rev int32 [m]): the unfiltered matches of both directions.  np.argmin returns the first of equal minima: the
    lowest index."""
    h, g = keys(q, t)
    return h.argmin(axis=1).astype(np.int32), g.argmin(axis=1).astype(np.int32)


def match(q, t, mutual=False, both=None):
    """(idx int32 [n], d2 float32 [n], forward int32 [n], rev int32 [m]): the contract's outputs and directions(q, t), which a caller that
    has them already passes as `both`."""
    q, t = np.asarray(q, np.float32), np.asarray(t, np.float32)
    fwd, rev = both if both is not None else directions(q, t)
    idx = fwd.copy()
    if mutual:
        idx[rev[fwd] != np.arange(len(q))] = -1
    d2 = np.full(len(q), np.inf, np.float32)
    kept = idx >= 0
    d = q[kept].astype(np.float64) - t[idx[kept]].astype(np.float64)
    s = np.zeros(int(kept.sum()))
    for b in range(q.shape[1]):
        s = s + d[:, b] * d[:, b]
    d2[kept] = s.astype(np.float32)
    return idx, d2, fwd, rev


def d2_float64(q, t, idx):
    """float64 squared distances of the kept matches (math.fsum-free: the sum of at most 64 non-negative terms in float64 is within
    64 * 2^-53 relative of the exact one, far below the fp32 rounding it is compared at)"""
    kept = idx >= 0
    d = np.asarray(q, np.float64)[kept] - np.asarray(t, np.float64)[idx[kept]]
    return kept, (d * d).sum(axis=1)
