"""mi_ransac_hypotheses and mi_ransac_register beyond the one planted call of tests/test_gpu_ransac.py: K24 (ransac_count_kernel) on a second
trip over its tile, on a partial tile behind a full one and on its unsplit plan; hypothesis indices beyond 2^16 and 2^18 through the
draws and K25's packed key, its tie rule over more than a thousand workgroups; 126 000 correspondences through K26; clouds away from the
origin with n != m; a call whose winner explains no pair; refinement to its limit of 8 passes; draws whose 64-bit sum wraps; a small call
behind a large one.  The cases and the proof that each is what it is named for: tests/ransac_scale_cases.py,
tests/test_ransac_scale_regimes.py.

No bound is new and none is taken from what the device gives:
  triples        equal
  valid          equal, except hypotheses the restatement calls fragile, at most 0.1 % of them (none for `no_inliers`)
  pose           ransac_scale_cases.check_poses, which tests/test_gpu_ransac.py calls too (the criteria of tests/kabsch_catalogue.py), here
                 in its two halves: objective, entries and t in one test, |R^T R - I| and |det R - 1| <= 32 eps in another
  inlier_count   within ransac_reference.count_rule's [lo, hi] of the float64 recount under the DEVICE's fp32 pose, lo == hi for 99 %
  winner         the arg-max of the same parameters' dump, the lowest h among equals
  refined pose   ransac_scale_cases.check_refined_pose over the mask of the step before, as tests/test_gpu_ransac.py does
  rmse           within 2^-23 relative of float64
  repeats, windows, a fixed point of the refinement, a small call behind a large one: equal bits"""
import collections

import numpy as np
import pytest

import ransac_reference as R
import ransac_scale_cases as S

pytestmark = pytest.mark.gpu

IDENTITY = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float32)
REGISTERED = tuple(n for n in S.CASES if n != "no_inliers")
Winner = collections.namedtuple("Winner", "best nvalid pose12 count")


def params(capi, c, **kw):
    return capi.ransac_params(c.max_distance, hypotheses=c.hypotheses, seed=c.seed, edge_similarity=c.edge_similarity, **kw)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def same_bits(a, b):
    """two outputs of the same entry point, array by array and scalar by scalar"""
    return len(a) == len(b) and all(np.array_equal(bits(np.asarray(x)), bits(np.asarray(y))) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def dump(ctx, capi):
    """name -> (triples, valid, pose12, counts) of the case's range first .. first + count - 1, each call made once"""
    cache = {}

    def run(name):
        if name not in cache:
            c = S.case(name)
            cache[name] = ctx.ransac_hypotheses(c.src, c.tgt, c.idx, params(capi, c), first=c.first, count=c.count)
        return cache[name]
    return run


@pytest.fixture(scope="module")
def winner(ctx, capi, dump):
    """name -> what the dump of ALL hypotheses of the case's parameters says the call returns: the valid hypothesis with the most inliers,
    the lowest h among equals; the number of valid ones; the winner's pose and count"""
    cache = {}

    def run(name):
        if name not in cache:
            c = S.case(name)
            # (`wrap` dumps a window: its whole range is dumped here and dropped again, 2^22 rows)
            triples, valid, pose12, counts = dump(name) if c.count == c.hypotheses else ctx.ransac_hypotheses(c.src, c.tgt, c.idx, params(capi, c))
            key = np.where(valid != 0, counts.astype(np.int64), -1)
            best = int(np.argmax(key))                          # argmax: the first of equal maxima
            cache[name] = Winner(best, int((valid != 0).sum()), pose12[best].copy(), int(counts[best]))
        return cache[name]
    return run


@pytest.fixture(scope="module")
def register(ctx, capi):
    """(name, refine) -> the outputs of mi_ransac_register with that many refinement passes and the mask, each call made once"""
    cache = {}

    def run(name, refine):
        if (name, refine) not in cache:
            c = S.case(name)
            cache[name, refine] = ctx.ransac_register(c.src, c.tgt, c.idx, params(capi, c, refine_iterations=refine), want_mask=True)
        return cache[name, refine]
    return run


# ---- 1. every hypothesis of every case
@pytest.mark.parametrize("name", S.CASES)
def test_triples_flags_and_poses(dump, name):
    c, ref = S.case(name), S.restated(name)
    triples, valid, pose12, counts = dump(name)
    assert len(valid) == c.count and np.array_equal(triples, ref["triples"])
    firm = ~ref["fragile"]
    assert ref["fragile"].sum() <= (0 if name == "no_inliers" else c.count // 1000)
    assert np.array_equal(valid[firm] != 0, ref["valid"][firm])
    bad = valid == 0
    assert (pose12[bad] == IDENTITY).all() and (counts[bad] == 0).all()
    S.check_poses_against_float64(valid, pose12, ref)


@pytest.mark.parametrize("name", S.CASES)
def test_every_valid_pose_is_a_rotation_to_32_eps(dump, name):
    """The bound of tests/test_gpu_ransac.py, |R^T R - I| <= 32 eps and |det R - 1| <= 32 eps, over thousands of poses.  This test found
    kabsch_rotation's own R at up to 45.6 eps (its Jacobi sweeps never re-orthonormalise U and V: `offset` 45.6 and 34.0 eps,
    `many_hypotheses` 39.0 and 32.2, `unsplit` 38.3 and 37.5, `no_inliers` 31.6 and 35.5, a few poses in a thousand each, where the 198
    valid poses of the planted call stay at 26.8 and 23.8); K23 now takes one Newton-Schulz step in fp64 behind the solve (mi_slam.h)."""
    triples, valid, pose12, counts = dump(name)
    S.check_orthogonality(valid, pose12, name)


@pytest.mark.parametrize("name", S.CASES)
def test_counts_equal_a_float64_recount_under_the_device_pose(dump, name):
    """the assertion that reaches K24's second trip, its partial tile behind a full one and its unsplit plan"""
    c = S.case(name)
    triples, valid, pose12, counts = dump(name)
    i, s, t = S.pairs(name)
    v = valid != 0
    lo, hi = S.recount(pose12[v], s, t, c.max_distance)
    off = np.flatnonzero((counts[v] < lo) | (counts[v] > hi))
    assert len(off) == 0, (name, np.flatnonzero(v)[off][:8], counts[v][off][:8], lo[off][:8], hi[off][:8])
    assert (lo == hi).mean() >= 0.99
    print("%s: %d valid, counts up to %d, lo == hi for %d" % (name, v.sum(), counts.max(), (lo == hi).sum()))
    if name == "no_inliers":
        assert hi.max() == 0


# ---- 2. the whole call
def check_call(c, out, win):
    """winner, count, mask and rmse of one mi_ransac_register against the dump and the float64 recount under the returned pose; returns
    the returned pose in the dump's layout"""
    i, s, t = S.pairs(c.name)
    Rr, tr, inl, rmse, best, nvalid, mask = out
    assert best == win.best and nvalid == win.nvalid
    pose = np.concatenate([Rr.T.reshape(9), tr])[None]
    lo, hi, d2 = R.count_rule(pose, s, t, c.max_distance)
    assert lo[0] == hi[0] == inl == int(mask.sum()) and (mask[c.idx < 0] == 0).all()
    assert np.array_equal(mask[i] != 0, d2[0] <= float(np.float32(c.max_distance)) ** 2)
    if inl > 0:
        want = np.sqrt(d2[0][mask[i] != 0].sum() / inl)
        assert abs(float(rmse) - want) <= 2.0 ** -23 * want
    else:
        assert np.isposinf(rmse)
    return pose[0]


def check_pass(c, out, before):
    """a call with at least one refinement pass: its pose is mi_kabsch over `before`, the mask of the step before by rank; and, on a
    planted problem, every true pair is an inlier and every point is within max_distance of its true image"""
    i, s, t = S.pairs(c.name)
    Rr, tr, mask = out[0], out[1], out[6]
    S.check_refined_pose(Rr, tr, s, t, before)
    moved = c.src.astype(np.float64) @ Rr.astype(np.float64).T + tr
    assert (mask[c.true] != 0).all()
    assert np.linalg.norm(moved - (c.src.astype(np.float64) @ c.R0.T + c.t0), axis=1).max() <= c.max_distance


def mask_under(c, pose12):
    """the float64 inlier flags by rank under one fp32 pose, decided for every pair"""
    i, s, t = S.pairs(c.name)
    lo, hi, d2 = R.count_rule(pose12[None], s, t, c.max_distance)
    assert lo[0] == hi[0]
    return d2[0] <= float(np.float32(c.max_distance)) ** 2


@pytest.mark.parametrize("refine", (0, 1, 2))
@pytest.mark.parametrize("name", REGISTERED)
def test_register(register, winner, name, refine):
    """for `many_pairs` K26 runs ransac_mask_kernel over 493 workgroups and ransac_sum_kernel over 493 trips per lane"""
    c, win = S.case(name), winner(name)
    out = register(name, refine)
    pose = check_call(c, out, win)
    if refine == 0:
        assert np.array_equal(bits(pose), bits(win.pose12)) and out[2] == win.count
        return
    i = S.pairs(name)[0]
    check_pass(c, out, mask_under(c, win.pose12) if refine == 1 else register(name, refine - 1)[6][i] != 0)


def test_refinement_to_the_limit(register, winner):
    """Every number of passes up to MI_RANSAC_MAX_REFINE on the planted problem: pass r is the Kabsch solve over the mask of pass r - 1;
    once a pass leaves the mask as it was, the next one sums the same rows in the same fixed order and solves the same system, so pose,
    count, rmse and mask repeat bit for bit from there on."""
    c, win = S.case("planted"), winner("planted")
    i = S.pairs("planted")[0]
    outs = [register("planted", r) for r in range(9)]
    fixed = None
    for r, out in enumerate(outs):
        check_call(c, out, win)
        if r == 0:
            continue
        check_pass(c, out, mask_under(c, win.pose12) if r == 1 else outs[r - 1][6][i] != 0)
        if fixed is None and np.array_equal(out[6], outs[r - 1][6]):
            fixed = r
    print("the mask stays from pass %s on" % fixed)
    assert fixed is not None and fixed < 8              # six hundred true pairs a tenth of max_distance from their images: settled at once
    for r in range(fixed + 1, 9):
        assert same_bits(outs[r], outs[fixed]), r


def test_a_winner_that_explains_no_pair(ctx, capi, dump):
    """mi_slam.h: refinement runs while at least 3 inliers remain, so a winner with fewer keeps its own pose; with none the mask is empty
    and rmse is +INFINITY beside a pose that is not the identity"""
    c = S.case("no_inliers")
    triples, valid, pose12, counts = dump(c.name)
    assert (counts == 0).all() and valid.sum() > 0
    lowest = int(np.argmax(valid != 0))
    for refine in (0, 2):
        Rr, tr, inl, rmse, best, nvalid, mask = ctx.ransac_register(c.src, c.tgt, c.idx, params(capi, c, refine_iterations=refine), want_mask=True)
        assert nvalid == int((valid != 0).sum()) > 0 and best == lowest
        assert inl == 0 and mask.sum() == 0 and np.isposinf(rmse)
        pose = np.concatenate([Rr.T.reshape(9), tr])
        assert np.array_equal(bits(pose), bits(pose12[lowest])) and not np.array_equal(pose, IDENTITY)


# ---- 3. windows, repeats, and a small call behind a large one
@pytest.mark.parametrize("name", ("many_hypotheses", "unsplit"))
def test_windows_and_repeats(ctx, capi, dump, name):
    """A window has workgroups of its own and, being short, another chunk plan: its rows are the whole dump's all the same.  The integer
    atomicAdd that merges the chunks may arrive in any order and does not show."""
    c = S.case(name)
    full = dump(name)
    again = ctx.ransac_hypotheses(c.src, c.tgt, c.idx, params(capi, c))
    assert same_bits(full, again)
    for first, count in ((65530, 12),) + (((262144, 1),) if name == "unsplit" else ()):
        window = ctx.ransac_hypotheses(c.src, c.tgt, c.idx, params(capi, c), first=first, count=count)
        assert same_bits(window, [a[first:first + count] for a in full]), (first, count)


def test_a_small_call_behind_a_large_one(ctx, capi):
    """the buffers have grown, and the tails of the mask and of the squared distances are stale"""
    small, large = S.case("planted"), S.case("many_pairs")

    def run():
        return (ctx.ransac_hypotheses(small.src, small.tgt, small.idx, params(capi, small)) +
                ctx.ransac_register(small.src, small.tgt, small.idx, params(capi, small, refine_iterations=2), want_mask=True))
    before = run()
    out = ctx.ransac_register(large.src, large.tgt, large.idx, params(capi, large, refine_iterations=2), want_mask=True)
    assert out[2] >= 30000
    assert same_bits(before, run())
