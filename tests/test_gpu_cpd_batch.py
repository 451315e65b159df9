"""GPU suite: mi_cpd_register_batch against the single call.

Every comparison is BIT EQUALITY (floats viewed as uint32) of sR, t, scale, the iteration count and the error between the batched call
and, per problem, a fresh mi_cpd_register on the same context: the reference is the existing, separately tested path.  Where the
single call returns a non-finite value (one moving point makes the scale 0/0 -- the CPU oracle returns NaN there too) the batched
value must be non-finite in the same entries and the bits are compared on the finite ones.  The stop reason has no single-call
output to compare with; it is checked against the rules in the order cpd_solve_kernel tests them (cap, tolerance, sigma^2)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import cpd_batch_catalogue as cat
from conftest import GOLD, check_measured

pytestmark = pytest.mark.gpu

STOP_MAX_ITERATIONS, STOP_TOLERANCE, STOP_SIGMA = 2, 5, 6


def singles(ctx, problems, params):
    return [ctx.cpd_register(b, a, params) for b, a in problems]      # sR, t, scale, iterations, error


def batch(ctx, problems, params):
    return ctx.cpd_register_batch([b for b, _ in problems], [a for _, a in problems], params)


def same_bits(x, y):
    x, y = np.ascontiguousarray(x, np.float32).reshape(-1), np.ascontiguousarray(y, np.float32).reshape(-1)
    fx, fy = np.isfinite(x), np.isfinite(y)
    return bool(np.array_equal(fx, fy) and np.array_equal(x[fx].view(np.uint32), y[fy].view(np.uint32)))


def assert_same(out, refs, label=""):
    sR, t, scale, it, err, why, _ = out
    assert len(refs) == len(it)
    bad = []
    for k, (sRs, ts, scs, its, errs) in enumerate(refs):
        same = (same_bits(sR[k], sRs) and same_bits(t[k], ts) and same_bits(scale[k], np.float32(scs)) and int(it[k]) == its
                and same_bits(err[k], np.float32(errs)))
        if not same:
            bad.append((k, int(it[k]), its, float(err[k]), errs, float(scale[k]), scs, float(np.abs(sR[k] - sRs).max()), float(np.abs(t[k] - ts).max())))
    assert not bad, "%s: %d of %d problems differ; (k, it, it_single, err, err_single, scale, scale_single, |dsR|, |dt|): %s" % (label, len(bad), len(refs), bad[:6])


def assert_reasons(out, params, label=""):
    """MAX_ITERATIONS exactly when iterations == cap; SIGMA only with error <= eps; error > eps below the cap means TOLERANCE."""
    _, _, _, it, err, why, _ = out
    cap, eps = params.max_iterations, params.eps
    for k in range(len(it)):
        i, e, w = int(it[k]), float(err[k]), int(why[k])
        assert w in (STOP_MAX_ITERATIONS, STOP_TOLERANCE, STOP_SIGMA), (label, k, w)
        if cap <= 0:
            assert i == 0 and w == STOP_MAX_ITERATIONS, (label, k, i, w)      # the loop condition fails before the first iteration
            continue
        assert (w == STOP_MAX_ITERATIONS) == (i == cap), (label, k, i, cap, w)
        if i == 0:
            assert w == STOP_SIGMA, (label, k, w)                             # sigma^2_0 <= eps: the error still holds its initial 1e5
            continue
        if w == STOP_SIGMA:
            assert not (e > eps), (label, k, e, eps)                          # (error <= eps; a collapsed, non-finite sigma^2 fails `> eps` too)
        if np.isfinite(e) and e > eps and i < cap:
            assert w == STOP_TOLERANCE, (label, k, i, e, w)


def check(ctx, problems, params, label, fallback=0):
    out = batch(ctx, problems, params)
    assert (out[6].problems_fallback, out[6].problems_batched) == (fallback, len(problems) - fallback), label
    assert_same(out, singles(ctx, problems, params), label)
    assert_reasons(out, params, label)
    return out


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


@pytest.fixture(scope="module")
def valu_ctx(capi):
    """A context whose single path contracts on the vector pipe (MISLAM_CPD_MFMA=0): other roundings than the batched kernel's chain."""
    os.environ["MISLAM_CPD_MFMA"] = "0"
    try:
        c = capi.Context(0)
    finally:
        del os.environ["MISLAM_CPD_MFMA"]
    yield c
    c.close()


def routing_edge(capi, p):
    n = 1
    while capi.cpd_batch_route(n, n, p):
        n += 1
        assert n < 10 ** 6
    return n - 1


# ---- 1
def test_one_problem_alone_and_in_a_pair(ctx, capi, rules_problems):
    p = capi.cpd_params(max_iterations=30)
    refs = singles(ctx, rules_problems[:2], p)
    out1 = batch(ctx, rules_problems[:1], p)
    assert (out1[6].problems_batched, out1[6].problems_fallback) == (1, 0) and out1[6].launches >= 1
    assert_same(out1, refs[:1], "B = 1")
    assert_same(batch(ctx, rules_problems[:2], p), refs, "B = 2")
    assert_same(batch(ctx, rules_problems[1::-1], p), refs[::-1], "B = 2 swapped")


# ---- 2
def test_all_size_combinations(ctx, capi):
    problems = cat.sizes_batch()
    assert len(problems) == 196
    out = check(ctx, problems, capi.cpd_params(max_iterations=30), "sizes")
    assert np.median(out[3]) >= 10, out[3]


def test_chunk_count_edges_up_to_the_routing_edge(ctx, capi):
    p = capi.cpd_params(max_iterations=12)
    edge = routing_edge(capi, p)
    assert edge >= 1024 and edge % 64 == 0
    check(ctx, cat.chunk_edge_batch(edge), p, "chunk edges")
    corner = [cat.pair(31, edge, edge), cat.pair(32, edge - 1, edge), cat.pair(33, edge, 1), cat.pair(34, 1, edge)]
    check(ctx, corner, p, "the routing edge from inside")


def test_a_registration_that_spans_several_launches(ctx, capi):
    """A launch carries a bounded number of EM iterations (clamp(2^26 / max m n, 4, 64): 16 at the routed edge); here the largest problems need
    more than one launch carries, so they are resumed from their state blocks, while a problem that stops at its first iteration (one moving
    point: the scale is 0/0) and a small one that stops early are found finished when the kernel is launched again."""
    p = capi.cpd_params(max_iterations=30, tolerance=0.0, eps=1e-4)
    edge = routing_edge(capi, p)
    per_launch = max(4, min(64, (1 << 26) // (edge * edge)))
    problems = [cat.pair(41, edge, edge), cat.pair(42, 1, 300), cat.pair(43, edge - 1, edge), cat.pair(44, 200, 300), cat.pair(45, edge, edge - 1)]
    refs = singles(ctx, problems, p)
    assert min(refs[k][3] for k in (0, 2, 4)) > per_launch, [r[3] for r in refs]      # three problems cross a launch boundary
    assert refs[1][3] < 4, refs[1][3]                                                 # one ends inside any first launch (at least 4 iterations)
    out = check(ctx, problems, p, "several launches")
    assert out[6].launches >= 2, out[6].launches
    assert out[6].launches == -(-max(r[3] for r in refs) // per_launch), (out[6].launches, [r[3] for r in refs])
    # the same through a permutation: which workgroup resumes and which returns at once changes, the bits do not
    order = [3, 0, 1, 4, 2]
    out = batch(ctx, [problems[i] for i in order], p)
    assert_same(out, [refs[i] for i in order], "several launches, permuted")
    assert out[6].launches >= 2


# ---- 3
def test_rules(ctx, capi, rules_problems):
    check(ctx, rules_problems, capi.cpd_params(max_iterations=40), "default with a cap")
    some = rules_problems[:12]
    for const_scale in (0, 1):
        for weight in (0.1, 0.3, 0.7, 0.0, -1.0, 1.0, 2.5):
            for sigma2_init in (0.0, 0.05):
                p = capi.cpd_params(const_scale=const_scale, weight=weight, sigma2_init=sigma2_init, max_iterations=25)
                check(ctx, some, p, "const_scale %d weight %g sigma2_init %g" % (const_scale, weight, sigma2_init))
    # sigma2_mode CPU_SEQUENTIAL is moot once sigma^2_0 is given: routed, and the same bits
    p = capi.cpd_params(sigma2_mode=capi.SIGMA2_CPU_SEQUENTIAL, sigma2_init=0.05, max_iterations=25)
    check(ctx, some, p, "sequential sigma2 mode with a given sigma2_init")


@pytest.mark.parametrize("max_iterations", [-1, 0, 1, 7])
def test_max_iterations(ctx, capi, rules_problems, max_iterations):
    p = capi.cpd_params(max_iterations=max_iterations)
    out = check(ctx, rules_problems, p, "max_iterations = %d" % max_iterations)
    assert (out[6].launches == 0) == (max_iterations <= 0)
    if max_iterations <= 0:                          # the initial state, as the single call returns it
        assert np.all(out[3] == 0) and np.all(out[2] == 1.0) and np.all(out[4] == np.float32(1e5))


def test_sync_every_moves_no_bit(ctx, capi, rules_problems):
    refs = singles(ctx, rules_problems, capi.cpd_params(max_iterations=30))
    for sync_every in (0, 1, 5):
        p = capi.cpd_params(max_iterations=30, sync_every=sync_every)
        assert_same(batch(ctx, rules_problems, p), refs, "sync_every %d" % sync_every)
        assert_same(batch(ctx, rules_problems[:4], capi.cpd_params(max_iterations=30)), singles(ctx, rules_problems[:4], p), "single call sync_every %d" % sync_every)


# ---- 4
def test_every_stop_reason(ctx, capi, oracle, rules_problems):
    seen = set()
    p = capi.cpd_params(max_iterations=3)
    out = check(ctx, rules_problems, p, "cap")
    assert np.all(out[5] == STOP_MAX_ITERATIONS) and np.all(out[3] == 3)
    seen.add(STOP_MAX_ITERATIONS)
    # tolerance = 0 with eps = 1e-3: only sigma^2 can stop the loop below the cap
    p = capi.cpd_params(max_iterations=60, tolerance=0.0, eps=1e-3)
    out = check(ctx, rules_problems, p, "sigma only")
    assert np.all(out[5] == STOP_SIGMA) and np.all(out[3] < 60) and np.all(out[4] <= 1e-3) and np.all(np.isfinite(out[4])), (out[3], out[5])
    seen.add(STOP_SIGMA)
    out = check(ctx, rules_problems, capi.cpd_params(max_iterations=60, tolerance=0.0, eps=1e-4), "sigma only, eps 1e-4")
    assert np.all(out[5] == STOP_SIGMA) and np.all(out[3] < 60)
    # eps = 0 with tolerance = 2e-2: only the tolerance can -- as long as sigma^2 stays a positive number.  A run that drives sigma^2 to 0 or
    # 0/0 before the tolerance fires fails `sigma^2 > 0` and stops on STOP_SIGMA in the single call too (DESIGN.md, K-batch CPD): it says
    # nothing about either path.  So this rule set gets a catalogue of its own, 40 problems picked by the CPU oracle, not by the device: the
    # first 40 of 80 seeded candidates that the oracle stops within 34 iterations (the span over which the tolerance fires on this family
    # of problems; later stops are runs on their way to the collapse) with a finite, positive sigma^2.  The reason is pinned on all 40.
    p = capi.cpd_params(max_iterations=60, tolerance=2e-2, eps=0.0)
    sound = []
    for b, a in list(rules_problems) + cat.rules_batch(seed=26000, count=40):
        r = oracle.cpd(b, a, eps=0.0, weight=p.weight, const_scale=False, max_iterations=60, tolerance=2e-2)
        if r[2] <= 34 and np.isfinite(r[3]) and r[3] > 0:
            sound.append((b, a))
        if len(sound) == 40:
            break
    assert len(sound) == 40
    out = check(ctx, sound, p, "tolerance only")
    assert np.all(out[5] == STOP_TOLERANCE) and np.all(out[3] < 60) and np.all(np.isfinite(out[4])) and np.all(out[4] > 0), (out[3], out[5])
    check(ctx, rules_problems, p, "eps = 0 on the whole rules catalogue, collapsing runs included")
    seen.add(STOP_TOLERANCE)
    out = check(ctx, rules_problems, capi.cpd_params(max_iterations=60, tolerance=2e-2, eps=1e-5), "tolerance before sigma")
    assert STOP_TOLERANCE in set(out[5].tolist())
    assert seen == {STOP_MAX_ITERATIONS, STOP_TOLERANCE, STOP_SIGMA}


# ---- 5
def test_permutation_permutes_the_outputs(ctx, capi, rules_problems):
    p = capi.cpd_params(max_iterations=30)
    refs = singles(ctx, rules_problems, p)
    perm = np.random.default_rng(3).permutation(len(rules_problems))
    assert_same(batch(ctx, [rules_problems[i] for i in perm], p), [refs[i] for i in perm], "permuted")


def test_more_problems_than_resident_workgroups(ctx, capi):
    problems = cat.small_batch()
    assert len(problems) == 1500 and max(max(len(b), len(a)) for b, a in problems) <= 256
    p = capi.cpd_params(max_iterations=20)
    refs = singles(ctx, problems, p)
    out = batch(ctx, problems, p)
    assert out[6].problems_batched == 1500
    assert_same(out, refs, "1500 small problems")
    assert_reasons(out, p, "1500 small problems")
    assert_same(batch(ctx, problems[700:701], p), refs[700:701], "one of them alone")


def test_overlapping_ranges(ctx, capi):
    p = capi.cpd_params(max_iterations=20)
    fixed = cat.pair(4000, 10, 900)[1]
    movings = [cat.pair(4000, 200 + 11 * k, 900)[0] for k in range(64)]           # same seed: the same surface as `fixed`
    before = np.concatenate(movings)
    counts = np.array([len(m) for m in movings])
    br = np.stack([np.cumsum(counts) - counts, counts], 1)
    ar = np.tile(np.array([[0, len(fixed)]]), (64, 1))
    out = ctx.cpd_register_batch(before, fixed, p, before_range=br, after_range=ar)
    assert_same(out, [ctx.cpd_register(m.copy(), fixed.copy(), p) for m in movings], "64 moving clouds, one fixed range")
    moving = movings[5]
    big = cat.pair(4000, 10, 2000)[1]
    ar = np.array([[17 * k, 500 + 5 * k] for k in range(64)])
    br = np.tile(np.array([[0, len(moving)]]), (64, 1))
    out = ctx.cpd_register_batch(moving, big, p, before_range=br, after_range=ar)
    assert_same(out, [ctx.cpd_register(moving.copy(), big[o:o + c].copy(), p) for o, c in ar], "one moving range, 64 fixed windows")


# ---- 6
def test_mixed_routing(ctx, capi, rules_problems):
    p = capi.cpd_params(max_iterations=15)
    edge = routing_edge(capi, p)
    problems = list(rules_problems[:30])
    problems.insert(7, cat.pair(11, edge + 1, edge + 1))
    problems.insert(20, cat.pair(12, 20000, 20000))
    check(ctx, problems, p, "mixed routing", fallback=2)
    q = capi.cpd_params(max_iterations=15, approximation=capi.CPD_APPROX_HYBRID)
    check(ctx, rules_problems[:6], q, "hybrid: all fallback", fallback=6)


def test_a_context_under_the_valu_contraction_takes_the_single_path(valu_ctx, ctx, capi, rules_problems):
    p = capi.cpd_params(max_iterations=30)
    some = rules_problems[:8]
    assert all(capi.cpd_batch_route(len(b), len(a), p) == 1 for b, a in some)      # the pure route function knows no context
    out = check(valu_ctx, some, p, "MISLAM_CPD_MFMA=0: all fallback", fallback=len(some))
    assert out[6].launches == 0
    # (the switch does move the single path's bits -- that is why the batched kernel must not run there)
    default = singles(ctx, some, p)
    assert any(not same_bits(out[0][k], default[k][0]) for k in range(len(some)))


# ---- 7
def test_ill_posed_inputs(ctx, ieee_ctx, capi):
    problems = [(b, a) for _, b, a in cat.ill_posed()]
    for c in (ctx, ieee_ctx):
        for p in (capi.cpd_params(max_iterations=20), capi.cpd_params(max_iterations=20, const_scale=1)):
            out = batch(c, problems, p)
            assert out[6].problems_fallback == 0
            assert_same(out, singles(c, problems, p), "ill-posed")


def test_rules_on_the_ieee_context(ieee_ctx, capi, rules_problems):
    check(ieee_ctx, rules_problems, capi.cpd_params(max_iterations=30), "MISLAM_SVD_IEEE=1")


# ---- 8
def test_no_state_leaks_between_calls(ctx, capi, rules_problems):
    p = capi.cpd_params(max_iterations=30)
    q = capi.cpd_params(max_iterations=9, const_scale=1, weight=0.5)
    first, second = rules_problems[:20], rules_problems[20:]
    ref_first_p, ref_second_q, ref_first_q = singles(ctx, first, p), singles(ctx, second, q), singles(ctx, first, q)
    assert_same(batch(ctx, first, p), ref_first_p, "call 1")
    assert_same(batch(ctx, second, q), ref_second_q, "call 2 (other rules, other sizes)")
    one = ctx.cpd_register(*rules_problems[3], p)
    b, a = rules_problems[5]
    ctx.icp_register(b, a, capi.icp_params(max_iterations=5))
    assert_same(batch(ctx, first, q), ref_first_q, "call 3, after a single CPD call and a single ICP call")
    assert_same(batch(ctx, rules_problems[3:4], p), [one], "the single call's problem")
    with pytest.raises(capi.MiSlamError):            # the batched call leaves no ICP problem loaded
        ctx.icp_run(1)


def test_empty_batch_and_invalid_arguments(ctx, capi, rules_problems):
    p = capi.cpd_params(max_iterations=20)
    out = ctx.cpd_register_batch([], [], p)
    assert len(out[3]) == 0 and (out[6].problems_batched, out[6].problems_fallback, out[6].launches) == (0, 0, 0)
    b, a = rules_problems[0]
    ok = np.array([[0, len(b)]]), np.array([[0, len(a)]])
    for br, ar in ((np.array([[5, len(b)]]), ok[1]), (ok[0], np.array([[0, len(a) + 1]])), (np.array([[0, -3]]), ok[1]), (ok[0], np.array([[-1, 10]])),
                   (np.array([[0, 0]]), ok[1])):
        with pytest.raises(capi.MiSlamError, match="error -1"):
            ctx.cpd_register_batch(b, a, p, before_range=br, after_range=ar)
    for kw in (dict(approximation=7), dict(estep_mode=5), dict(sigma2_mode=9), dict(approximation=capi.CPD_APPROX_FULL, fgt_order_of_truncation=0),
               dict(approximation=capi.CPD_APPROX_HYBRID, estep_mode=1)):
        with pytest.raises(capi.MiSlamError, match="error -1"):
            ctx.cpd_register_batch([b], [a], capi.cpd_params(max_iterations=5, **kw))
        with pytest.raises(capi.MiSlamError, match="error -1"):     # ... as the single call refuses them
            ctx.cpd_register(b, a, capi.cpd_params(max_iterations=5, **kw))
    with pytest.raises(capi.MiSlamError, match="error -1"):         # the FGT modes need two points per cloud
        ctx.cpd_register_batch([b, b[:1]], [a, a], capi.cpd_params(max_iterations=5, approximation=capi.CPD_APPROX_FULL))
    # a NULL output through the raw entry point; the message names the problem for a bad range in the middle of a batch
    T = np.zeros(32, np.float32)
    it, why = np.zeros(2, np.int32), np.zeros(2, np.int32)
    err = np.zeros(2, np.float32)
    br2 = np.array([[0, 10], [0, 10]], np.int32)
    args = lambda T_, it_, err_, why_, bad: capi.cpd_register_batch_raw(ctx._h, 2, b.ctypes.data, bad.ctypes.data, a.ctypes.data, br2.ctypes.data, C.addressof(p),
                                                                         T_, None, it_, err_, why_, None)
    assert args(None, it.ctypes.data, err.ctypes.data, why.ctypes.data, br2) == capi.MI_ERR_INVALID_ARG
    assert args(T.ctypes.data, None, err.ctypes.data, why.ctypes.data, br2) == capi.MI_ERR_INVALID_ARG
    assert args(T.ctypes.data, it.ctypes.data, None, why.ctypes.data, br2) == capi.MI_ERR_INVALID_ARG
    assert args(T.ctypes.data, it.ctypes.data, err.ctypes.data, None, br2) == capi.MI_ERR_INVALID_ARG
    assert args(T.ctypes.data, it.ctypes.data, err.ctypes.data, why.ctypes.data, np.array([[0, 10], [0, -1]], np.int32)) == capi.MI_ERR_INVALID_ARG
    assert b"problem 1" in capi.lib().mi_last_error()
    assert args(T.ctypes.data, it.ctypes.data, err.ctypes.data, why.ctypes.data, br2) == capi.MI_OK      # out_scale and info may be NULL
    # a negative problem count, NULL clouds, NULL range arrays
    raw = lambda n_, b_, br_, a_, ar_: capi.cpd_register_batch_raw(ctx._h, n_, b_, br_, a_, ar_, C.addressof(p), T.ctypes.data, None, it.ctypes.data,
                                                                    err.ctypes.data, why.ctypes.data, None)
    assert raw(-1, b.ctypes.data, br2.ctypes.data, a.ctypes.data, br2.ctypes.data) == capi.MI_ERR_INVALID_ARG
    assert raw(2, None, br2.ctypes.data, a.ctypes.data, br2.ctypes.data) == capi.MI_ERR_INVALID_ARG
    assert raw(2, b.ctypes.data, br2.ctypes.data, None, br2.ctypes.data) == capi.MI_ERR_INVALID_ARG
    assert raw(2, b.ctypes.data, None, a.ctypes.data, br2.ctypes.data) == capi.MI_ERR_INVALID_ARG
    assert raw(2, b.ctypes.data, br2.ctypes.data, a.ctypes.data, None) == capi.MI_ERR_INVALID_ARG
    assert capi.cpd_register_batch_raw(ctx._h, 2, b.ctypes.data, br2.ctypes.data, a.ctypes.data, br2.ctypes.data, None, T.ctypes.data, None,
                                       it.ctypes.data, err.ctypes.data, why.ctypes.data, None) == capi.MI_ERR_INVALID_ARG      # NULL parameters
    assert_same(batch(ctx, rules_problems[:2], p), singles(ctx, rules_problems[:2], p), "a valid call after the refused ones")


def test_a_distributed_context_is_refused(capi, rules_problems):
    with capi.Context(0, 0, 1, exchange=lambda array, kind: None) as dist:      # one rank over the caller's transport: distributed all the same
        with pytest.raises(capi.MiSlamError, match="error %d" % capi.MI_ERR_STATE):
            batch(dist, rules_problems[:2], capi.cpd_params(max_iterations=5))
        out = dist.cpd_register(*rules_problems[0], capi.cpd_params(max_iterations=5))     # the single call runs there
        assert out[3] == 5


# ---- 9
def test_catalogue_against_the_oracle(ctx, capi, oracle, rules_problems):
    p = capi.cpd_params(max_iterations=50)
    sR, t, scale, it, err, why, _ = batch(ctx, rules_problems, p)
    worst = 0.0
    for k, (b, a) in enumerate(rules_problems):
        Ro, to, ito, eo = oracle.cpd(b, a, eps=p.eps, weight=p.weight, const_scale=False, max_iterations=50, tolerance=p.tolerance)
        assert int(it[k]) == ito and ito < 50, (k, int(it[k]), ito)
        worst = max(worst, float(np.sqrt(((sR[k] - Ro) ** 2).sum() + ((t[k] - to) ** 2).sum())))
    check_measured("cpd_batch_rules40_vs_oracle", worst, 1e-4, floor=2e-6)        # the bar of the single call's bunny test
    # ... and 2x what was measured when this suite was written (tests/golden/cpd_batch_measured.json, this suite's own fixture)
    measured = json.load(open(os.path.join(GOLD, "cpd_batch_measured.json")))["values"]["cpd_batch_rules40_vs_oracle"]
    assert worst <= 2.0 * measured + 2e-6, (worst, measured)
