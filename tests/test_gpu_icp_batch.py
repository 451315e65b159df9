"""GPU suite: mi_icp_register_batch against the single call.

Every comparison is BIT EQUALITY of the transform (R and t as uint32; the other four entries of out_T are the constants 0, 0, 0, 1 in
both calls), the iteration count, the error (as uint32) and the stop reason, between the batched call and, per problem, a fresh
mi_icp_register + mi_icp_result on the same context: the reference is the existing, separately tested path."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import icp_batch_catalogue as cat
from conftest import GOLD, check_measured

pytestmark = pytest.mark.gpu

STOP_CONVERGED, STOP_MAX_ITERATIONS, STOP_NO_PAIRS, STOP_ERROR_INCREASED = 1, 2, 3, 4


def single(ctx, b, a, params):
    ctx.icp_register(b, a, params)
    return ctx.icp_result()                      # R, t, iterations, error, stop_reason


def singles(ctx, problems, params):
    return [single(ctx, b, a, params) for b, a in problems]


def batch(ctx, problems, params):
    return ctx.icp_register_batch([b for b, _ in problems], [a for _, a in problems], params)


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def assert_same(out, refs, label=""):
    R, t, it, err, why, _ = out
    assert len(refs) == len(it)
    bad = []
    for k, (Rs, ts, its, errs, whys) in enumerate(refs):
        same = (np.array_equal(bits(R[k]), bits(Rs)) and np.array_equal(bits(t[k]), bits(ts)) and int(it[k]) == its
                and bits(err[k:k + 1])[0] == bits(np.float32(errs).reshape(1))[0] and int(why[k]) == whys)
        if not same:
            bad.append((k, int(it[k]), its, float(err[k]), errs, int(why[k]), whys, float(np.abs(R[k] - Rs).max()), float(np.abs(t[k] - ts).max())))
    assert not bad, "%s: %d of %d problems differ; (k, it, it_single, err, err_single, why, why_single, |dR|, |dt|): %s" % (label, len(bad), len(refs), bad[:6])


@pytest.fixture(scope="module")
def sizes_problems():
    return cat.sizes_batch()


@pytest.fixture(scope="module")
def rules_problems():
    return cat.rules_batch()


@pytest.fixture(scope="module")
def ieee_ctx(capi):
    """A context whose 3 x 3 SVDs run in IEEE divisions and roots (MISLAM_SVD_IEEE=1; switches are read at context creation)."""
    os.environ["MISLAM_SVD_IEEE"] = "1"
    try:
        c = capi.Context(0)
    finally:
        del os.environ["MISLAM_SVD_IEEE"]
    yield c
    c.close()


# ---- 5 (first: the smallest batches)
def test_one_problem_alone_and_in_a_pair(ctx, capi, rules_problems):
    p = capi.icp_params(max_iterations=60)
    refs = singles(ctx, rules_problems[:2], p)
    out1 = batch(ctx, rules_problems[:1], p)
    assert (out1[5].problems_batched, out1[5].problems_fallback) == (1, 0) and out1[5].launches >= 1
    assert_same(out1, refs[:1], "B = 1")
    assert_same(batch(ctx, rules_problems[:2], p), refs, "B = 2")
    assert_same(batch(ctx, rules_problems[1::-1], p), refs[::-1], "B = 2 swapped")


# ---- 1
def test_all_size_combinations(ctx, capi, sizes_problems):
    p = capi.icp_params(max_iterations=60)
    refs = singles(ctx, sizes_problems, p)
    out = batch(ctx, sizes_problems, p)
    assert out[5].problems_batched == len(sizes_problems) == 196 and out[5].problems_fallback == 0     # no problem of this catalogue may take the fallback
    assert_same(out, refs, "sizes")
    its = np.array([r[2] for r in refs])
    assert np.median(its) >= 10 and its.max() <= 60, its


# ---- 2
def rule_sets(capi):
    sets = [("default", capi.icp_params(max_iterations=80)), ("cuda_slam", capi.icp_params(cuda_slam=True, max_iterations=80))]
    for dist in (capi.DIST_CPU_ROUNDING, capi.DIST_FMA):
        for compose in (capi.COMPOSE_CPU_ADDITIVE, capi.COMPOSE_EXACT):
            for filt in (0, 1):
                sets.append(("d%d_c%d_f%d" % (dist, compose, filt),
                             capi.icp_params(dist_mode=dist, compose_mode=compose, filter_pairs=filt, max_iterations=80, max_distance_squared=0.05)))
    return sets


def test_rules(ctx, capi, rules_problems):
    for name, p in rule_sets(capi):
        assert_same(batch(ctx, rules_problems, p), singles(ctx, rules_problems, p), name)


def test_unbounded_default_rules(ctx, capi):
    # max_iterations = -1 as the presets have it, on problems dense enough to converge under eps = 1e-3
    problems = [cat.pair(6000 + k, 3000 + 100 * k, 3500) for k in range(8)]
    for p in (capi.icp_params(), capi.icp_params(cuda_slam=True)):
        refs = singles(ctx, problems, p)
        assert all(r[4] in (STOP_CONVERGED, STOP_ERROR_INCREASED) for r in refs)
        assert_same(batch(ctx, problems, p), refs, "max_iterations = -1")


@pytest.mark.parametrize("max_iterations", [0, 1, 7])
def test_max_iterations(ctx, capi, rules_problems, max_iterations):
    p = capi.icp_params(max_iterations=max_iterations)
    out = batch(ctx, rules_problems, p)
    assert_same(out, singles(ctx, rules_problems, p), "max_iterations = %d" % max_iterations)
    assert (out[5].launches == 0) == (max_iterations == 0)


def test_sync_every_and_nn_mode_move_no_bit(ctx, capi, rules_problems):
    base = capi.icp_params(max_iterations=40)
    refs = singles(ctx, rules_problems, base)
    for sync_every in (0, 1, 5):
        for nn_mode in (capi.NN_AUTO, capi.NN_BRUTEFORCE, capi.NN_TREE, capi.NN_GRID):
            p = capi.icp_params(max_iterations=40, sync_every=sync_every, nn_mode=nn_mode)
            assert_same(batch(ctx, rules_problems, p), refs, "sync_every %d nn_mode %d" % (sync_every, nn_mode))
    # and the single call under the other searches is the same reference (the header's promise, checked here on three problems)
    for nn_mode in (capi.NN_TREE, capi.NN_GRID):
        p = capi.icp_params(max_iterations=40, nn_mode=nn_mode)
        assert_same(batch(ctx, rules_problems[:3], base), singles(ctx, rules_problems[:3], p), "single call nn_mode %d" % nn_mode)


# ---- 3
def test_every_stop_reason(ctx, capi):
    seen = {}
    for name, b, a, kw in cat.stop_reason_problems():
        p = capi.icp_params(**kw)
        ref = single(ctx, b, a, p)
        assert_same(batch(ctx, [(b, a)], p), [ref], name)
        seen.setdefault(ref[4], []).append(name)
    for reason in (STOP_CONVERGED, STOP_MAX_ITERATIONS, STOP_NO_PAIRS, STOP_ERROR_INCREASED):
        assert reason in seen, "the catalogue no longer reaches stop reason %d: %s" % (reason, seen)
    # the aborting problems as ONE batch under their common rules
    ab = [(b, a) for name, b, a, kw in cat.stop_reason_problems() if name.startswith("abort")]
    p = capi.icp_params(cuda_slam=True, eps=1e-7, max_iterations=200)
    refs = singles(ctx, ab, p)
    assert STOP_ERROR_INCREASED in [r[4] for r in refs]
    assert_same(batch(ctx, ab, p), refs, "abort batch")


# ---- 4
def test_ill_posed_solves(ctx, ieee_ctx, capi):
    problems = [(b, a) for _, b, a in cat.ill_posed()]
    for c in (ctx, ieee_ctx):
        for p in (capi.icp_params(max_iterations=30), capi.icp_params(cuda_slam=True, max_iterations=30)):
            out = batch(c, problems, p)
            assert out[5].problems_fallback == 0
            assert_same(out, singles(c, problems, p), "ill-posed")


def test_all_sizes_on_the_ieee_context(ieee_ctx, capi, sizes_problems):
    p = capi.icp_params(max_iterations=60)
    out = batch(ieee_ctx, sizes_problems, p)
    assert out[5].problems_batched == 196
    assert_same(out, singles(ieee_ctx, sizes_problems, p), "sizes, MISLAM_SVD_IEEE=1")


# ---- 5
def test_permutation_permutes_the_outputs(ctx, capi, rules_problems):
    p = capi.icp_params(max_iterations=50)
    refs = singles(ctx, rules_problems, p)
    perm = np.random.default_rng(3).permutation(len(rules_problems))
    assert_same(batch(ctx, [rules_problems[i] for i in perm], p), [refs[i] for i in perm], "permuted")


def test_more_problems_than_resident_workgroups(ctx, capi):
    problems = cat.small_batch()
    assert len(problems) == 1500 and max(max(len(b), len(a)) for b, a in problems) <= 512
    p = capi.icp_params(max_iterations=40)
    refs = singles(ctx, problems, p)
    out = batch(ctx, problems, p)
    assert out[5].problems_batched == 1500
    assert_same(out, refs, "1500 small problems")
    assert_same(batch(ctx, problems[700:701], p), refs[700:701], "one of them alone")


def test_overlapping_ranges(ctx, capi):
    p = capi.icp_params(max_iterations=40)
    fixed = cat.pair(4000, 10, 3000)[1]
    movings = [cat.pair(4000, 200 + 13 * k, 3000)[0] for k in range(64)]          # same seed: the same surface as `fixed`
    before = np.concatenate(movings)
    counts = np.array([len(m) for m in movings])
    br = np.stack([np.cumsum(counts) - counts, counts], 1)
    ar = np.tile(np.array([[0, len(fixed)]]), (64, 1))
    out = ctx.icp_register_batch(before, fixed, p, before_range=br, after_range=ar)
    assert_same(out, [single(ctx, m.copy(), fixed.copy(), p) for m in movings], "64 moving clouds, one fixed range")
    # one moving range against 64 fixed clouds, themselves overlapping windows of one array
    moving = movings[5]
    big = cat.pair(4000, 10, 4096)[1]
    ar = np.array([[17 * k, 2000 + 5 * k] for k in range(64)])
    br = np.tile(np.array([[0, len(moving)]]), (64, 1))
    out = ctx.icp_register_batch(moving, big, p, before_range=br, after_range=ar)
    assert_same(out, [single(ctx, moving.copy(), big[o:o + c].copy(), p) for o, c in ar], "one moving range, 64 fixed windows")


# ---- 6
def test_mixed_routing(ctx, capi, rules_problems):
    p = capi.icp_params(max_iterations=30)
    n = 1
    while capi.icp_batch_route(n, n, p):
        n += 1
        assert n < 10 ** 6
    problems = list(rules_problems[:30])
    problems.insert(7, cat.pair(11, n, n))
    problems.insert(20, cat.pair(12, 20000, 20000))
    out = batch(ctx, problems, p)
    assert (out[5].problems_fallback, out[5].problems_batched) == (2, 30)
    assert_same(out, singles(ctx, problems, p), "mixed routing")


# ---- 7
def test_no_state_leaks_between_calls(ctx, capi, rules_problems):
    p = capi.icp_params(max_iterations=50)
    q = capi.icp_params(cuda_slam=True, max_iterations=9)
    first, second = rules_problems[:20], rules_problems[20:]
    ref_first_p, ref_second_q, ref_first_q = singles(ctx, first, p), singles(ctx, second, q), singles(ctx, first, q)
    assert_same(batch(ctx, first, p), ref_first_p, "call 1")
    assert_same(batch(ctx, second, q), ref_second_q, "call 2 (other rules, other sizes)")
    one = single(ctx, *rules_problems[3], p)
    assert_same(batch(ctx, first, q), ref_first_q, "call 3, after a single call")
    assert_same(batch(ctx, rules_problems[3:4], p), [one], "the single call's problem")
    with pytest.raises(capi.MiSlamError):            # the batched call leaves no problem loaded
        ctx.icp_run(1)


def test_empty_batch_and_invalid_arguments(ctx, capi, rules_problems):
    p = capi.icp_params(max_iterations=20)
    out = ctx.icp_register_batch([], [], p)
    assert len(out[2]) == 0 and (out[5].problems_batched, out[5].problems_fallback, out[5].launches) == (0, 0, 0)
    b, a = rules_problems[0]
    ok = np.array([[0, len(b)]]), np.array([[0, len(a)]])
    for br, ar in ((np.array([[5, len(b)]]), ok[1]), (ok[0], np.array([[0, len(a) + 1]])), (np.array([[0, -3]]), ok[1]), (ok[0], np.array([[-1, 10]])),
                   (np.array([[0, 0]]), ok[1])):
        with pytest.raises(capi.MiSlamError, match="error -1"):
            ctx.icp_register_batch(b, a, p, before_range=br, after_range=ar)
    # a NULL output through the raw entry point; the message names the problem for a bad range in the middle of a batch
    T = np.zeros(32, np.float32)
    it, why = np.zeros(2, np.int32), np.zeros(2, np.int32)
    err = np.zeros(2, np.float32)
    br2 = np.array([[0, 10], [0, 10]], np.int32)
    args = lambda T_, it_, bad: capi.icp_register_batch_raw(ctx._h, 2, b.ctypes.data, bad.ctypes.data, a.ctypes.data, br2.ctypes.data, C.addressof(p),
                                                             T_, it_, err.ctypes.data, why.ctypes.data, None)
    assert args(None, it.ctypes.data, br2) == capi.MI_ERR_INVALID_ARG
    assert args(T.ctypes.data, None, br2) == capi.MI_ERR_INVALID_ARG
    assert args(T.ctypes.data, it.ctypes.data, np.array([[0, 10], [0, -1]], np.int32)) == capi.MI_ERR_INVALID_ARG
    assert b"problem 1" in capi.lib().mi_last_error()
    assert_same(batch(ctx, rules_problems[:2], p), singles(ctx, rules_problems[:2], p), "a valid call after the refused ones")


# ---- 8
def test_catalogue_against_the_oracle(ctx, capi, oracle, rules_problems):
    p = capi.icp_params(max_iterations=80)
    R, t, it, err, why, _ = batch(ctx, rules_problems, p)
    worst = 0.0
    for k, (b, a) in enumerate(rules_problems):
        Ro, to, ito, eo = oracle.icp(b, a, 1e-3, 1000.0, 80)
        assert int(it[k]) == ito, (k, int(it[k]), ito)
        worst = max(worst, float(np.sqrt(((R[k] - Ro) ** 2).sum() + ((t[k] - to) ** 2).sum())))
    check_measured("icp_batch_rules40_vs_oracle", worst, 1e-4, floor=2e-6)       # the bar of the bunny / synth tests of the single call
    # ... and 2x what was measured when this suite was written (tests/golden/icp_batch_measured.json, this suite's own fixture)
    measured = json.load(open(os.path.join(GOLD, "icp_batch_measured.json")))["values"]["icp_batch_rules40_vs_oracle"]
    assert worst <= 2.0 * measured + 2e-6, (worst, measured)
