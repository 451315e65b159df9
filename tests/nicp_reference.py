"""A float64 restatement of the stages of the non-iterative registration (csrc/nicp_api.hip, K10) in plain numpy: no device, no oracle.
Shared by tests/test_nicp_reference.py (CPU: pins this file against oracle/nicp_oracle.c) and tests/test_gpu_nicp_stages.py (the device's
stages against it).

  moments(b, a)                  (sums [32], sums of the terms' magnitudes [32]) in the layout of the comment at NICP_SUMS: every point taken
                                 about the FIRST point of its cloud, the terms formed in float64 exactly as the kernel forms them (the
                                 differences are exact; a product of two of them is one fp64 rounding, the same one on the device), summed in
                                 np.longdouble.  about_first=False: the raw coordinates (what the kernel summed before it took an origin)
  centred(b, a)                  dict(cb, ca, Gb, Ga, Saa, Sab, pairs) from clouds centred FIRST, in float64: nothing cancels
  sums_from_raw(s, m, n)         the same quantities the way the host forms them from the 32 sums, sum x x^T - n c c^T: what cancels
  axes(G)                        (U [3, 3] columns by descending eigenvalue, eigenvalues, relative gaps (l0 - l1) / l0 and (l1 - l2) / l0)
  approx_error(R, b, a)          mean_i |a'_i - R b'_i|^2 over the index-wise pairs, from the centred points
  exact_error(R32, t32, sub, after, limit)   the subcloud score of one candidate: fp32 transform in the kernel's operation order, the every-pair
                                 nearest neighbour in MI_DIST_CPU_ROUNDING keys (launch_nn runs with fma = 0), the float64 mean of the d2 < limit
  store_if_optimal, driver       the list quirks and the pick on given numbers (common/nicputils.cpp:5-26, noniterative.cpp:204-282)
  full_permutation(heads, size)  a permutation of 0..size-1 that starts with the three heads (the rest in ascending order)"""
import numpy as np

import knn_reference as K
import plane_reference as P

U64 = 2.0 ** -53
EPS32 = 2.0 ** -23
NICP_SUMS = 32
MOMENT_BLOCKS_CAP = 512                    # ICP_MAX_PARTIAL_BLOCKS: icp_reduce_blocks(n) = min(ceil(n / 256), 512)
ONE_PASS = MOMENT_BLOCKS_CAP * 256         # the largest cloud the moments grid covers in one trip of its grid-stride loop
SYM = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
MODE_NONE, MODE_FULL, MODE_HYBRID = 0, 1, 2
FLT_MAX = np.float32(np.finfo(np.float32).max)


def _f64(x):
    return np.ascontiguousarray(np.asarray(x, np.float32).astype(np.float64)).reshape(-1, 3)


def _sum(v):
    return np.sum(np.asarray(v, np.longdouble), axis=0)


def moments(b, a, about_first=True):
    b, a = _f64(b), _f64(a)
    if about_first:
        b, a = b - b[0], a - a[0]                                     # exact: fp32 values in fp64
    m, n = len(b), len(a)
    p = min(m, n)
    ap, bp = a[:p], b[:p]
    cols = []
    for x in (b, a):
        cols += [x[:, d] for d in range(3)] + [x[:, i] * x[:, j] for i, j in SYM]
    cols += [ap[:, d] for d in range(3)]
    cols.append((ap[:, 0] * ap[:, 0] + ap[:, 1] * ap[:, 1]) + ap[:, 2] * ap[:, 2])
    cols += [ap[:, r] * bp[:, c] for r in range(3) for c in range(3)]
    cols.append(np.zeros(1))
    assert len(cols) == NICP_SUMS
    return (np.array([_sum(c) for c in cols], np.longdouble), np.array([_sum(np.abs(c)) for c in cols], np.longdouble))


def centred(b, a):
    b, a = _f64(b), _f64(a)
    m, n = len(b), len(a)
    p = min(m, n)
    cb, ca = np.asarray(_sum(b) / m, np.float64), np.asarray(_sum(a) / n, np.float64)
    bc, ac = b - cb, a - ca
    return dict(cb=cb, ca=ca, Gb=bc.T @ bc, Ga=ac.T @ ac, Saa=float((ac[:p] ** 2).sum()), Sab=ac[:p].T @ bc[:p], pairs=p, m=m, n=n)


def sums_from_raw(s, m, n):
    """The host's formula (nicp_api.hip sums_from_raw) in float64 on 32 sums about any origin: centroids ABOUT THAT ORIGIN, Gb, Ga, Saa, Sab."""
    s = np.asarray(s, np.float64)
    cb, ca = s[0:3] / m, s[9:12] / n
    sym = np.array([[0, 1, 2], [1, 3, 4], [2, 4, 5]])
    Gb = s[3 + sym] - m * np.outer(cb, cb)
    Ga = s[12 + sym] - n * np.outer(ca, ca)
    p = min(m, n)
    Saa = s[21] - 2.0 * (ca[0] * s[18] + ca[1] * s[19] + ca[2] * s[20]) + p * (ca[0] * ca[0] + ca[1] * ca[1] + ca[2] * ca[2])
    Sab = s[22:31].reshape(3, 3) - np.outer(ca, s[0:3]) - np.outer(s[18:21], cb) + p * np.outer(ca, cb)
    return dict(cb=cb, ca=ca, Gb=Gb, Ga=Ga, Saa=float(Saa), Sab=Sab, pairs=p, m=m, n=n)


def approx_from_sums(R, c):
    """(Saa + tr(R^T R Gb) - 2 <R, Sab>) / m, the host's expansion, on a dict of centred() / sums_from_raw()."""
    R = np.asarray(R, np.float64)
    return float((c["Saa"] + np.trace(R.T @ R @ c["Gb"]) - 2.0 * (R * c["Sab"]).sum()) / c["m"])


def axes(G):
    lam, U = np.linalg.eigh(np.asarray(G, np.float64))
    lam, U = lam[::-1].copy(), U[:, ::-1].copy()
    return U, lam, np.array([(lam[0] - lam[1]) / lam[0], (lam[1] - lam[2]) / lam[0]])


def approx_error(R, b, a):
    """mean over the m points of `before` of |a'_i - R b'_i|^2, i < m <= n (the modes that read this error refuse m > n, and the device's
    pair sums do not define it there)."""
    R = np.asarray(R, np.float64)
    b, a = _f64(b), _f64(a)
    c = centred(b, a)
    p = c["pairs"]
    assert p == len(b)
    d = (a[:p] - c["ca"]) - (b - c["cb"]) @ R.T
    return float(_sum((d * d).sum(axis=1)) / len(b))


def approx_floor(c):
    """What the expansion can lose against approx_error: (m + 8) 2^-53 (Saa + tr Gb + 2 |Sab|_1) / m, the three terms it adds."""
    return (c["m"] + 8) * U64 * (c["Saa"] + np.trace(c["Gb"]) + 2.0 * np.abs(c["Sab"]).sum()) / c["m"]


def transform(R32, t32, cloud):
    """float32: ((R0 x + R3 y) + R6 z) + t, one rounding per operation (nicp_transform_kernel); R32 indexed [row, col]."""
    R32, t32 = np.asarray(R32), np.asarray(t32)
    assert R32.dtype == np.float32 and t32.dtype == np.float32
    return P.move_f32(R32, t32, cloud)


def exact_error(R32, t32, sub, after, limit=1e6):
    """-> (float64 mean of the nearest d2 < limit -- nan when none is --, the count kept, idx [sn], d2 float32 [sn])."""
    cur = transform(R32, t32, sub)
    idx, d2, _ = K.knn(cur, after, 1, K.DIST_CPU_ROUNDING)
    idx, d2 = idx[:, 0], d2[:, 0]
    keep = d2 < np.float32(limit)
    kept = int(keep.sum())
    mean = float(_sum(d2[keep].astype(np.float64)) / kept) if kept else float("nan")
    return mean, kept, idx, d2


def store_if_optimal(lst, cand, approx, desired):
    """lst: list of (candidate, approx).  A result that beats several stored ones is inserted before each of them in turn; the list is cut back
    only when an insertion overflows it; an equal error beats nothing.  -> True when the list overflowed."""
    len0 = len(lst)
    if len0 == 0 and desired > 0:
        lst.append((cand, approx))
        return False
    for i in range(len0):
        if approx < lst[i][1]:
            lst.insert(i, (cand, approx))
            if len(lst) > desired:
                del lst[desired:]
                return True
    return False


def driver(cands, approx_errors, exact_errors, eps, mode):
    """cands: the candidates' labels in repetition order; approx_errors / exact_errors: float32 per candidate (exact_errors may be a callable
    label -> error, asked only for the candidates the driver scores).  -> dict(repetitions, winner (a label, None without a candidate), error,
    scored (labels in scoring order), listed (the ranked list's labels), overflowed (an insertion cut the list back)).  Where no scored candidate's error compares below FLT_MAX (0 / 0: no
    point within the limit) the winner is the first candidate scored and the error FLT_MAX -- the product's contract (mi_slam.h); the reference
    leaves the pair uninitialised there."""
    ask = exact_errors if callable(exact_errors) else (lambda k: exact_errors[k])
    eps = np.float32(eps)
    reps = len(cands)
    winner, min_error, scored, listed, overflowed = None, FLT_MAX, [], [], False
    for rep, k in enumerate(cands):
        if mode == MODE_NONE:
            e = np.float32(ask(k))
            scored.append(k)
            if rep == 0:
                winner = k
            if e < min_error:
                min_error, winner = e, k
                if min_error <= eps:
                    return dict(repetitions=rep + 1, winner=k, error=e, scored=scored, listed=[], overflowed=False)
        else:
            overflowed |= store_if_optimal(listed, k, np.float32(approx_errors[k]), 5 if mode == MODE_HYBRID else 1)
    if mode != MODE_NONE:
        for i, (k, _) in enumerate(listed):
            e = np.float32(ask(k))
            scored.append(k)
            if i == 0:
                winner = k
            if e < min_error:
                min_error, winner = e, k
                if min_error <= eps:
                    return dict(repetitions=reps, winner=k, error=e, scored=scored, listed=[x[0] for x in listed], overflowed=overflowed)
    return dict(repetitions=reps, winner=winner, error=min_error, scored=scored, listed=[x[0] for x in listed], overflowed=overflowed)


def full_permutation(head, size):
    head = [int(h) for h in head]
    assert len(set(head)) == 3
    rest = [i for i in range(size) if i not in head]
    return np.array(head + rest, np.int32)


def permuted(b, a, perm):
    """ApplyPermutation (common.h:101-108): the first len(perm) entries of each cloud permuted, the rest of the larger cloud in place."""
    b, a = np.array(b, np.float32), np.array(a, np.float32)
    k = len(perm)
    b[:k], a[:k] = b[perm].copy(), a[perm].copy()
    return b, a


# ---- the clouds of the two test modules ----
SHIFT = np.array([100.0, -50.0, 25.0])


def rotation(angle=0.7):
    ax = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * Kx @ Kx


def rigid_pair(seed, m, n, noise, shift=None):
    """tests/test_nicp_oracle.rigid_pair with two sizes: max(m, n) points of an anisotropic Gaussian (3, 1.5, 0.7), `after` = R b + t + noise
    in the same point order; before = the first m, after = the first n.  shift: added to both clouds before the rounding to float32."""
    rng = np.random.default_rng(seed)
    top = max(m, n)
    b = rng.normal(size=(top, 3)) * np.array([3.0, 1.5, 0.7])
    a = b @ rotation().T + np.array([0.5, -1.0, 2.0]) + rng.normal(size=(top, 3)) * noise
    s = np.zeros(3) if shift is None else np.asarray(shift, np.float64)
    return (b[:m] + s).astype(np.float32), (a[:n] + s).astype(np.float32)


def loose_pair(seed, m, n, shift=None):
    """Two INDEPENDENT anisotropic Gaussians, each turned its own way: no candidate fits, every approximated error is of the clouds' size."""
    rng = np.random.default_rng(seed)
    b = (rng.normal(size=(m, 3)) * np.array([2.5, 1.2, 0.5])) @ rotation(0.4).T
    a = (rng.normal(size=(n, 3)) * np.array([0.6, 2.8, 1.3])) @ rotation(-1.1).T + np.array([-0.3, 0.8, 1.5])
    s = np.zeros(3) if shift is None else np.asarray(shift, np.float64)
    return (b + s).astype(np.float32), (a + s).astype(np.float32)


def min_gap(b, a):
    c = centred(b, a)
    return float(min(axes(c["Gb"])[2].min(), axes(c["Ga"])[2].min()))


# ---- the pick (tests g): heads that give each of the 8 sign patterns of the principal-axis alignment once, by ascending approximated error ----
# rigid_pair(m * 7 + n, m, n, 0.01); found by drawing triples until every pattern had shown (the patterns depend on the first three points only)
PICK_HEADS = {
    (257, 257): [[29, 111, 13], [73, 221, 12], [198, 175, 45], [210, 6, 14], [81, 74, 77], [7, 194, 130], [109, 129, 197], [71, 223, 101]],
    (1000, 2500): [[705, 649, 543], [529, 635, 927], [637, 166, 72], [162, 940, 17], [91, 200, 296], [672, 910, 985], [722, 125, 730], [244, 302, 541]],
}
# 9 repetitions each: eight different candidates and one row twice (a tie of every error).  "falling": every newcomer beats the whole list, the
# insertion quirk overflows the five; "mixed": the best candidate in the middle, the early exit of mode none has repetitions to skip
PICK_ORDERS = {"falling": [7, 6, 5, 4, 4, 3, 2, 1, 0], "mixed": [4, 7, 1, 1, 0, 6, 2, 5, 3]}
PICK_SUBCLOUD = {(257, 257): 64, (1000, 2500): 65}


def pick_case(m, n, order):
    """(before, after, heads [9, 3], subcloud_idx) of one case of the pick tests."""
    b, a = rigid_pair(m * 7 + n, m, n, 0.01)
    heads = np.array([PICK_HEADS[(m, n)][k] for k in PICK_ORDERS[order]], np.int32)
    sub = np.random.default_rng(m + n).permutation(m)[:PICK_SUBCLOUD[(m, n)]].astype(np.int32)
    return b, a, heads, sub


def near_ties(errors, labels, rel=2.0 ** -22):
    """Pairs of DIFFERENT candidates (labels: what makes two candidates the same, e.g. the bits of R | t) whose errors lie within rel of each other."""
    out = []
    for i in range(len(errors)):
        for j in range(i + 1, len(errors)):
            if labels[i] != labels[j] and abs(float(errors[i]) - float(errors[j])) <= rel * max(abs(float(errors[i])), abs(float(errors[j]))):
                out.append((i, j))
    return out
