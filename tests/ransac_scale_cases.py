"""The cases of tests/test_gpu_ransac_scale.py and what they share: problems at which ransac_count_kernel (K24) takes a second trip over its
tile, ends a chunk on a partial tile behind a full one, or walks all of C in one workgroup; hypothesis indices beyond 2^16 and 2^18;
126 000 correspondences; clouds away from the origin with n != m; a call without a single inlier; draws whose 64-bit sum wraps -- and the
restatement of K24's launch plan that tests/test_ransac_scale_regimes.py holds every case against, so that a case is shown to be what it
is named for without a device.  chunk_plan restates the arithmetic of ransac_chunk_len and ransac_count (csrc/ransac_kernels.hip) in
integers; it is not read from the library.

No tolerance is introduced here: check_poses (in its two halves) and check_refined_pose hold the bounds of tests/test_gpu_ransac.py (the criteria of
tests/kabsch_catalogue.py, the t bound of tests/test_gpu_kabsch3.py), and that file calls them too."""
import collections
import functools

import numpy as np

import ransac_reference as R
from kabsch_catalogue import EPS, kabsch64, objective_deficit, orthogonality, posedness

RANSAC_BLOCK = 256                   # csrc/kernels.h: hypotheses per workgroup of K23 - K25, pairs per tile of K24, ranks per workgroup of K26
MAX_GRID_Y = 65535
CU_COUNTS = range(1, 401)            # the CU counts over which every case is shown to stay in its regime (an MI355X has 256)
SLAB = 1 << 23                       # poses x pairs per slab of recount: the float64 [K, C] matrices stay at 64 MB each


def chunk_plan(H, C, cus):
    """(chunks, tiles per chunk, rows of the last tile of the last chunk) of K24 over H hypotheses and C pairs on `cus` CUs:
    ransac_chunk_len asks for ceil(2 cus / ceil(H / 256)) chunks, at least 1, at most one per tile and 65 535, and gives every chunk the
    same whole number of tiles; ransac_count launches as many chunks of that length as cover C."""
    blocks, tiles = -(-H // RANSAC_BLOCK), -(-C // RANSAC_BLOCK)
    wanted = max(1, min(-(-2 * cus // blocks), tiles, MAX_GRID_Y))
    per_chunk = -(-tiles // wanted)
    chunks = -(-C // (per_chunk * RANSAC_BLOCK))
    return chunks, per_chunk, C - (tiles - 1) * RANSAC_BLOCK


def last_chunk_tiles(H, C, cus):
    """the tiles of the last chunk, its partial one included"""
    chunks, per_chunk, _ = chunk_plan(H, C, cus)
    return -(-C // RANSAC_BLOCK) - (chunks - 1) * per_chunk


Case = collections.namedtuple("Case", "name src tgt idx hypotheses seed edge_similarity max_distance first count R0 t0 true")
CASES = ("many_hypotheses", "unsplit", "many_pairs", "many_pairs_loose", "offset", "no_inliers", "wrap")
OFFSET = (100.0, -50.0, 25.0)


def frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def planted(n=2000):
    """ransac_reference.planted() of n points, frozen"""
    src, tgt, idx, R0, t0, true = R.planted(n=n)
    return tuple(frozen(a) for a in (src, tgt, idx, R0, t0, true))


@functools.lru_cache(maxsize=None)
def case(name):
    """The case of a name in CASES, or "planted"; hypotheses first .. first + count - 1 of `hypotheses` are the ones dumped and restated
    (all of them except for `wrap`)."""
    src, tgt, idx, R0, t0, true = planted()
    H, seed, edge, maxd, first = 4096, 7, 0.9, 0.01, 0
    if name == "planted":                                     # tests/test_gpu_ransac.py's own call: one tile per chunk on 256 CUs
        pass
    elif name == "many_hypotheses":                           # C = 1 800: seven full tiles and one of 8 rows
        H = 70001
    elif name == "unsplit":                                   # C = 600: two full tiles and one of 88 rows; 1 025 workgroups of hypotheses
        idx = idx.copy()
        idx[np.flatnonzero(idx >= 0)[600:]] = -1
        true = true & (idx >= 0)
        H = 262145
    elif name in ("many_pairs", "many_pairs_loose"):          # C = 126 000: 492 full tiles and one of 48 rows
        src, tgt, idx, R0, t0, true = planted(140000)
        H, edge = 300, (0.9 if name == "many_pairs" else 0.0)
    elif name == "offset":                                    # the planted pose still maps one cloud onto the other; m = n + 500
        rng = np.random.default_rng(307)
        off = np.array(OFFSET)
        src = (src.astype(np.float64) + off).astype(np.float32)
        tgt = np.concatenate([(tgt.astype(np.float64) + R0 @ off).astype(np.float32),
                              (rng.uniform(-1, 1, (500, 3)) + R0 @ off + t0).astype(np.float32)])
    elif name == "no_inliers":                                # two unrelated clouds, every source point paired with a target of its own
        rng = np.random.default_rng(311)
        src, tgt = rng.uniform(-1, 1, (500, 3)).astype(np.float32), rng.uniform(-1, 1, (500, 3)).astype(np.float32)
        idx, true, R0, t0 = rng.permutation(500).astype(np.int32), np.zeros(500, bool), None, None
        H, edge, maxd = 512, 0.0, 1e-4
    elif name == "wrap":                                      # seed + GOLDEN (3 h + r + 1) passes 2^64 before it is mixed
        H, seed, first = 1 << 22, (1 << 64) - 1, (1 << 22) - 65
    else:
        raise KeyError(name)
    arrays = [frozen(np.ascontiguousarray(a)) for a in (src, tgt, idx)]
    return Case(name, *arrays, H, seed, edge, maxd, first, H - first, R0, t0, frozen(np.array(true)))


@functools.lru_cache(maxsize=None)
def pairs(name):
    """ransac_reference.correspondences of the case: (source index per rank, s, t)"""
    c = case(name)
    return tuple(frozen(a) for a in R.correspondences(c.src, c.tgt, c.idx))


@functools.lru_cache(maxsize=None)
def restated(name):
    """ransac_reference.hypotheses of the case's dumped range, worked once"""
    c = case(name)
    ref = R.hypotheses(c.src, c.tgt, c.idx, c.seed, c.first, c.count, c.edge_similarity)
    for a in ref.values():
        frozen(a)
    return ref


def restated_pose12(ref):
    """the restatement's float64 poses rounded to fp32, in the layout of mi_ransac_hypotheses (R9 column-major, then t3)"""
    return np.concatenate([ref["R64"].transpose(0, 2, 1).reshape(-1, 9), ref["t64"]], axis=1).astype(np.float32)


def recount(pose12, s, t, max_distance):
    """ransac_reference.count_rule's (lowest, highest possible count) of every pose, worked in slabs of at most SLAB pose-pair products"""
    pose12 = np.asarray(pose12, np.float32).reshape(-1, 12)
    step = max(1, min(4096, SLAB // len(s)))
    lo, hi = np.zeros(len(pose12), np.int64), np.zeros(len(pose12), np.int64)
    for k in range(0, len(pose12), step):
        lo[k:k + step], hi[k:k + step] = R.count_rule(pose12[k:k + step], s, t, max_distance)[:2]
    return lo, hi


def moments_h32(s, t):
    """the fp32-rounded cross-covariance of the pairs s -> t as the solve forms it from fp64 moments, as float64 [1, 3, 3]"""
    n = float(len(s))
    cb, ca = s.sum(axis=0) / n, t.sum(axis=0) / n
    return (t.T @ s - n * np.outer(ca, cb)).astype(np.float32).astype(np.float64)[None], cb, ca


def check_orthogonality(valid, pose12, what="poses"):
    """every pose of a dump finite, every valid one with |R^T R - I| and |det R - 1| at most 32 eps; prints the worst of each first"""
    v = valid != 0
    assert np.isfinite(pose12).all()
    e, de = orthogonality(pose12[v, :9].reshape(-1, 3, 3).transpose(0, 2, 1))
    print("%s: %d valid, |R^T R - I| up to %.1f eps (%d above 32), |det R - 1| up to %.1f eps (%d above 32)" % (
        what, v.sum(), e.max() / EPS, (e > 32 * EPS).sum(), de.max() / EPS, (de > 32 * EPS).sum()))
    assert e.max() <= 32 * EPS and de.max() <= 32 * EPS


def check_poses_against_float64(valid, pose12, ref):
    """Every valid pose of a dump against the float64 Kabsch of the same fp32-rounded H (ref: ransac_reference.hypotheses of the same
    range): the objective's deficit at most 16 eps, and, where well posed (at least half of them), R entry by entry within
    32 (eps sigma_1 / g + eps) and t within 3 |cb| dR + 8 eps (|ca| + 3 |cb|)."""
    v = valid != 0
    Rd = pose12[v, :9].reshape(-1, 3, 3).transpose(0, 2, 1)          # column-major -> [row, col]
    Hm, S, d, g = ref["H"][v], ref["S"][v], ref["d"][v], ref["g"][v]
    assert objective_deficit(Rd, Hm, S, d).max() <= 16 * EPS
    cond, well, _ = posedness(S, g)
    dR = np.abs(Rd.astype(np.float64) - ref["R64"][v]).max(axis=(1, 2))
    assert well.sum() >= 0.5 * v.sum() and (dR[well] <= 32 * (cond[well] + EPS)).all()
    cb, ca = ref["cb"][v], ref["ca"][v]
    tol = 3 * np.abs(cb).max(axis=1) * dR + 8 * EPS * (np.abs(ca).max(axis=1) + 3 * np.abs(cb).max(axis=1))
    assert (np.abs(pose12[v, 9:].astype(np.float64) - ref["t64"][v]).max(axis=1)[well] <= tol[well]).all()


def check_poses(valid, pose12, ref):
    """both of the above: what tests/test_gpu_ransac.py asks of every valid pose"""
    check_orthogonality(valid, pose12)
    check_poses_against_float64(valid, pose12, ref)


def check_refined_pose(Rr, tr, s, t, before):
    """A refined pose (Rr [3, 3], tr) is mi_kabsch over the pairs flagged in `before`, the mask of the step before, by rank: held to the
    criteria of tests/kabsch_catalogue.py against the float64 Kabsch of the fp32-rounded cross-covariance over exactly that mask."""
    assert before.sum() >= 3
    Hm, cb, ca = moments_h32(s[before], t[before])
    R64, S, d, g = kabsch64(Hm)
    e, de = orthogonality(Rr[None])
    assert e[0] <= 32 * EPS and de[0] <= 32 * EPS
    assert objective_deficit(Rr[None], Hm, S, d)[0] <= 16 * EPS
    cond, well, _ = posedness(S, g)
    assert well[0]                                         # hundreds of pairs in a cube: far from any tie
    dR = np.abs(Rr.astype(np.float64) - R64[0]).max()
    assert dR <= 32 * (cond[0] + EPS)
    tol = 3 * np.abs(cb).max() * dR + 8 * EPS * (np.abs(ca).max() + 3 * np.abs(cb).max())
    assert np.abs(tr.astype(np.float64) - (ca - R64[0] @ cb)).max() <= tol
