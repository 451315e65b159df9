"""GPU suite of mi_ransac_register / mi_ransac_hypotheses against the restatement of tests/ransac_reference.py, on the planted problem
(ransac_reference.planted: 2 000 points, 30 % true pairs, 60 % random, 10 % none, noise 1e-3, max_distance 0.01, H = 4 096).

The bounds (none of them taken from what the device gives):
  triples        equal
  valid          equal, except hypotheses the restatement calls fragile (an edge ratio within 1e-12 of the threshold, or sigma_2 of H below
                 1e-5 sigma_1), at most 0.1 % of them
  pose           by the criteria of tests/kabsch_catalogue.py against the float64 Kabsch of the same fp32-rounded H: the objective's deficit
                 at most 16 eps; |R^T R - I| and |det R - 1| at most 32 eps (about twenty fp32 plane rotations of one rounding each); entry
                 by entry within 32 (eps sigma_1 / g + eps) where that is at most 1e-4 (WELL_POSED); t within the bound of
                 tests/test_gpu_kabsch3.py, 3 |cb| dR + 8 eps (|ca| + 3 |cb|)
  inlier_count   equal to the float64 recount under the DEVICE's fp32 pose, an interval where a pair is within 1e-12 of the threshold
  refined pose   the same criteria against the float64 Kabsch over the mask of the step before
  rmse           within 2^-23 relative of float64"""
import functools

import numpy as np
import pytest

import ransac_reference as R
from ransac_scale_cases import check_poses, check_refined_pose

pytestmark = pytest.mark.gpu

H, SEED, MAXD = 4096, 7, 0.01


@functools.lru_cache(maxsize=None)
def problem():
    src, tgt, idx, R0, t0, true = R.planted()
    for a in (src, tgt, idx, true):
        a.setflags(write=False)
    return src, tgt, idx, R0, t0, true


@functools.lru_cache(maxsize=None)
def reference():
    src, tgt, idx = problem()[:3]
    return R.hypotheses(src, tgt, idx, SEED, 0, H, 0.9)


@pytest.fixture(scope="module")
def dumped(ctx, capi):
    src, tgt, idx = problem()[:3]
    return ctx.ransac_hypotheses(src, tgt, idx, capi.ransac_params(MAXD, hypotheses=H, seed=SEED))


def test_triples_and_valid_flags(dumped):
    triples, valid, pose12, counts = dumped
    ref = reference()
    assert np.array_equal(triples, ref["triples"])
    firm = ~ref["fragile"]
    assert ref["fragile"].sum() <= H // 1000
    assert np.array_equal(valid[firm] != 0, ref["valid"][firm])
    assert valid.sum() >= 50
    bad = valid == 0
    assert (pose12[bad] == np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float32)).all() and (counts[bad] == 0).all()


def test_every_valid_pose_against_float64(dumped):
    triples, valid, pose12, counts = dumped
    ref = reference()
    check_poses(valid, pose12, ref)


def test_counts_equal_a_float64_recount_under_the_device_pose(dumped):
    triples, valid, pose12, counts = dumped
    src, tgt, idx = problem()[:3]
    i, s, t = R.correspondences(src, tgt, idx)
    v = valid != 0
    lo, hi, _ = R.count_rule(pose12[v], s, t, MAXD)
    assert ((lo <= counts[v]) & (counts[v] <= hi)).all() and (lo == hi).mean() > 0.99
    assert (counts[v] >= 500).sum() >= 50


@pytest.fixture(scope="module")
def register(ctx, capi):
    """refine -> the outputs of mi_ransac_register on the planted problem with that many refinement passes, each call made once"""
    src, tgt, idx = problem()[:3]
    cache = {}

    def run(refine):
        if refine not in cache:
            cache[refine] = ctx.ransac_register(src, tgt, idx, capi.ransac_params(MAXD, hypotheses=H, seed=SEED, refine_iterations=refine), want_mask=True)
        return cache[refine]
    return run


@pytest.mark.parametrize("refine", (0, 1, 2))
def test_register(register, dumped, refine):
    triples, valid, pose12, counts = dumped
    src, tgt, idx, R0, t0, true = problem()
    i, s, t = R.correspondences(src, tgt, idx)
    Rr, tr, inl, rmse, best, nvalid, mask = register(refine)
    key = np.where(valid != 0, counts.astype(np.int64), -1)
    assert best == int(np.argmax(key)) and nvalid == int((valid != 0).sum())      # argmax: the first of equal maxima, the lowest h
    pose = np.concatenate([Rr.T.reshape(9), tr])[None]
    lo, hi, d2 = R.count_rule(pose, s, t, MAXD)
    assert lo[0] == hi[0] == inl == int(mask.sum()) and (mask[idx < 0] == 0).all()
    assert np.array_equal(mask[i] != 0, d2[0] <= float(np.float32(MAXD)) ** 2)
    want = np.sqrt(d2[0][mask[i] != 0].sum() / inl)
    assert abs(float(rmse) - want) <= 2.0 ** -23 * want
    if refine == 0:
        assert np.array_equal(pose[0], pose12[best]) and inl == counts[best]
        return
    # the pose is mi_kabsch over the mask of the step before: the recount under the dumped winner for the first pass, the mask the call
    # with one pass fewer returns for the second.  Held to the criteria of tests/kabsch_catalogue.py against the float64 Kabsch of the
    # fp32-rounded cross-covariance over exactly that mask
    if refine == 1:
        lo0, hi0, d20 = R.count_rule(pose12[best][None], s, t, MAXD)
        assert lo0[0] == hi0[0]
        before = d20[0] <= float(np.float32(MAXD)) ** 2
    else:
        before = register(refine - 1)[6][i] != 0
    check_refined_pose(Rr, tr, s, t, before)
    # the planted problem's condition: every true pair is an inlier, every point within max_distance of its true image
    moved = src.astype(np.float64) @ Rr.astype(np.float64).T + tr
    assert (mask[true] != 0).all()
    assert np.linalg.norm(moved - (src.astype(np.float64) @ R0.T + t0), axis=1).max() <= MAXD


def test_small_and_degenerate_cases(ctx, capi):
    src, tgt, idx = (np.array(a) for a in problem()[:3])
    three = np.full(len(idx), -1, np.int32)
    keep = np.flatnonzero(problem()[5])[:3]
    three[keep] = idx[keep]
    p = capi.ransac_params(MAXD, hypotheses=256, seed=1, edge_similarity=0.0, refine_iterations=0)
    triples, valid, pose12, counts = ctx.ransac_hypotheses(src, tgt, three, p)
    assert np.isin(triples, keep).all() and 20 <= valid.sum() <= 110 and (counts[valid != 0] == 3).all()     # 6 / 27 of the triples are distinct
    out = ctx.ransac_register(src, tgt, three, p, want_mask=True)
    assert out[2] == 3 and out[4] == int(np.argmax(valid != 0)) and out[6].sum() == 3
    # three collinear pairs: no valid hypothesis, the stated outputs
    line = np.zeros((3, 3), np.float32)
    line[:, 0] = [0, 1, 2]
    Rr, tr, inl, rmse, best, nvalid, mask = ctx.ransac_register(line, line + np.float32(1), np.arange(3, dtype=np.int32), p, want_mask=True)
    assert (nvalid, inl, best) == (0, 0, -1) and np.array_equal(Rr, np.eye(3, dtype=np.float32)) and (tr == 0).all() and np.isposinf(rmse) and mask.sum() == 0
    two = three.copy()
    two[keep[0]] = -1
    with pytest.raises(capi.MiSlamError) as e:
        ctx.ransac_register(src, tgt, two, p)
    assert "fewer than 3" in str(e.value)
    # H = 1 and H = 65 are prefixes of the same sequence; a window in the middle too
    full = ctx.ransac_hypotheses(src, tgt, idx, capi.ransac_params(MAXD, hypotheses=65, seed=SEED))
    for a, b in zip(full, dumped_prefix(ctx, capi, 65)):
        assert np.array_equal(a, b)
    one = ctx.ransac_hypotheses(src, tgt, idx, capi.ransac_params(MAXD, hypotheses=1, seed=SEED))
    assert all(np.array_equal(a, b[:1]) for a, b in zip(one, full))
    window = ctx.ransac_hypotheses(src, tgt, idx, capi.ransac_params(MAXD, hypotheses=65, seed=SEED), first=60, count=5)
    assert all(np.array_equal(a, b[60:]) for a, b in zip(window, full))
    # no edge check: only repeated ranks and collinear triples are invalid
    loose = ctx.ransac_hypotheses(src, tgt, idx, capi.ransac_params(MAXD, hypotheses=512, seed=SEED, edge_similarity=0.0))
    ref = R.hypotheses(src, tgt, idx, SEED, 0, 512, 0.0)
    assert np.array_equal(loose[1][~ref["fragile"]] != 0, ref["valid"][~ref["fragile"]]) and loose[1].sum() >= 500
    # two seeds, and the same seed twice
    other = ctx.ransac_hypotheses(src, tgt, idx, capi.ransac_params(MAXD, hypotheses=65, seed=SEED + 1))
    assert not np.array_equal(other[0], full[0])
    pr = capi.ransac_params(MAXD, hypotheses=H, seed=SEED)
    a, b = ctx.ransac_register(src, tgt, idx, pr, want_mask=True), ctx.ransac_register(src, tgt, idx, pr, want_mask=True)
    assert all(np.array_equal(np.asarray(x).view(np.uint8) if isinstance(x, np.ndarray) else np.asarray(x), np.asarray(y).view(np.uint8) if isinstance(y, np.ndarray) else np.asarray(y))
               for x, y in zip(a, b))


def dumped_prefix(ctx, capi, count):
    src, tgt, idx = problem()[:3]
    return ctx.ransac_hypotheses(src, tgt, idx, capi.ransac_params(MAXD, hypotheses=H, seed=SEED), first=0, count=count)


def raw(ctx, capi, src, n, tgt, m, idx, p, null_out=None):
    import ctypes as C
    R9, t3, scal, rmse, mask = np.full(9, -7.5, np.float32), np.full(3, -7.5, np.float32), np.full(3, -7, np.int32), np.full(1, -7.5, np.float32), np.full(max(n, 1), 7, np.uint8)
    outs = [R9.ctypes.data, t3.ctypes.data, scal[0:].ctypes.data, rmse.ctypes.data, scal[1:].ctypes.data, scal[2:].ctypes.data]
    if null_out is not None:
        outs[null_out] = None
    rc = capi.ransac_register_raw(ctx._h, None if src is None else src.ctypes.data, n, None if tgt is None else tgt.ctypes.data, m, None if idx is None else idx.ctypes.data,
                                  None if p is None else C.addressof(p), *outs, mask.ctypes.data)
    untouched = bool((R9 == -7.5).all() and (t3 == -7.5).all() and (scal == -7).all() and rmse[0] == -7.5 and (mask == 7).all())
    return rc, capi.lib().mi_last_error().decode(), untouched


def raw_hypotheses(ctx, capi, src, n, tgt, m, idx, p, first, count):
    import ctypes as C
    rows = max(min(count, 64), 1)
    tri, val, pose, cnt = np.full(3 * rows, -7, np.int32), np.full(rows, 7, np.uint8), np.full(12 * rows, -7.5, np.float32), np.full(rows, -7, np.int32)
    rc = capi.ransac_hypotheses_raw(ctx._h, None if src is None else src.ctypes.data, n, None if tgt is None else tgt.ctypes.data, m, None if idx is None else idx.ctypes.data,
                                    None if p is None else C.addressof(p), first, count, tri.ctypes.data, val.ctypes.data, pose.ctypes.data, cnt.ctypes.data)
    return rc, capi.lib().mi_last_error().decode(), bool((tri == -7).all() and (val == 7).all() and (pose == -7.5).all() and (cnt == -7).all())


def test_refusals_leave_the_outputs_untouched(ctx, capi):
    src, tgt, idx = (np.array(a) for a in problem()[:3])
    n = len(src)
    good = capi.ransac_params(MAXD, hypotheses=64)
    cases = [(None, n, tgt, n, idx, good), (src, n, None, n, idx, good), (src, n, tgt, n, None, good), (src, n, tgt, n, idx, None), (src, 0, tgt, n, idx, good), (src, n, tgt, 0, idx, good)]
    for kw in (dict(hypotheses=0), dict(hypotheses=(1 << 22) + 1), dict(edge_similarity=1.0), dict(edge_similarity=-0.1), dict(edge_similarity=float("nan")),
               dict(refine_iterations=-1), dict(refine_iterations=9)):
        cases.append((src, n, tgt, n, idx, capi.ransac_params(MAXD, **kw)))
    for md in (0.0, -1.0, float("inf"), float("nan")):
        cases.append((src, n, tgt, n, idx, capi.ransac_params(md)))
    for args in cases:
        rc, msg, untouched = raw(ctx, capi, *args)
        assert rc == capi.MI_ERR_INVALID_ARG and untouched and msg.startswith("mi_ransac_register: "), msg
    for value in (n, -2):
        bad = idx.copy()
        bad[1500], bad[700] = value, value
        rc, msg, untouched = raw(ctx, capi, src, n, tgt, n, bad, good)
        assert rc == capi.MI_ERR_INVALID_ARG and untouched and "idx[700] " in msg, msg
    for k in range(6):                                    # every required output
        rc, msg, untouched = raw(ctx, capi, src, n, tgt, n, idx, good, null_out=k)
        assert rc == capi.MI_ERR_INVALID_ARG and untouched and msg.startswith("mi_ransac_register: null output"), msg
    two = np.full(n, -1, np.int32)
    two[[5, 900]] = idx[[0, 1]].clip(0)
    rc, msg, untouched = raw(ctx, capi, src, n, tgt, n, two, good)
    assert rc == capi.MI_ERR_INVALID_ARG and untouched and msg == "mi_ransac_register: 2 correspondences, fewer than 3", msg
    bad = idx.copy()
    bad[700] = n
    for args in ((None, n, tgt, n, idx, good, 0, 4), (src, n, tgt, n, idx, None, 0, 4), (src, 0, tgt, n, idx, good, 0, 4), (src, n, tgt, n, two, good, 0, 4),
                 (src, n, tgt, n, bad, good, 0, 4), (src, n, tgt, n, idx, capi.ransac_params(0.0, hypotheses=64), 0, 4), (src, n, tgt, n, idx, good, 60, 5),
                 (src, n, tgt, n, idx, good, -1, 4), (src, n, tgt, n, idx, good, 0, 0)):
        rc, msg, untouched = raw_hypotheses(ctx, capi, *args)
        assert rc == capi.MI_ERR_INVALID_ARG and untouched and msg.startswith("mi_ransac_hypotheses: "), msg
    assert raw_hypotheses(ctx, capi, src, n, tgt, n, idx, good, 59, 5)[0] == capi.MI_OK
    with pytest.raises(capi.MiSlamError) as e:
        ctx.ransac_hypotheses(src, tgt, idx, good, first=60, count=5)
    assert str(e.value).find("mi_ransac_hypotheses: ") >= 0
