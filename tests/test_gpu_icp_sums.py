"""GPU suite: the 16 moments and 2 error sums of a point-to-point ICP iteration, from every producer and through every reducer, against the
float64 reference of tests/icp_sums_reference.py; the reported error, the solve and the composition against the same reference.

Every case runs whole iterations through icp_load / icp_run and reads what the last solve read (selftest_icp_schedule()["sums"]) and the
state (icp_result).  For iteration k the pose T_(k-1) comes from the same registration one iteration earlier (the library is deterministic to
the bit), cur = transform(before, T_(k-1)) is float32 operation by operation, the pairs are nn_search(cur, after, dist_mode, NN_BRUTEFORCE)
on another context (pinned bit for bit to the oracle by tests/test_gpu_nn.py) and use = d2 < max_distance_squared under filter_pairs.  The
moments are held to moments(cur, after[idx], use), the error sums to error_sums(after[idx], transform(before, T_k), use), both inside
icp_sums_reference.bounds -- k 2^-53 sum|term| with k counted from the code, nothing measured; the counts and every all-zero sum exactly.

Producers (asserted: the search kernel's name, the constants of kernels.h / nn_grid.h, the switch the context was created under, the
counting build's own counter, rank / world):
  helper     nn_grid_kernel<FUSED> with the helper wave (split_walks: n <= GRID_HELPER_FULL_MAX_POINTS)
  onewave    the same kernel, one wave per chunk (MISLAM_GRID_SPLIT_WALKS=0)
  counting   its counting build (mi_profile_search_stats on: one wave per chunk, the counters beside the sums)
  brute, tree   K2 icp_moments_rows_kernel + K4/K5 icp_transform_error_rows_kernel behind NN_BRUTEFORCE / NN_TREE
  world1     a distributed context of one rank: the fused kernel, the 64 reduced rows all-reduced, the solve from them
  stand-alone   mi_cross_moments / mi_kabsch / mi_transform_mse on the caller's pairs
Reducers (asserted from the schedule read-back: the one-workgroup form deals no work order, the ticket form leaves its cursors, the two-launch
form zeroes them): icp_reduce_solve_kernel up to ICP_FUSED_SOLVE_MAX_ROWS rows; icp_rows_reduce_solve_kernel beyond, and below under
MISLAM_ICP_FUSED_SOLVE=0; icp_rows_reduce_kernel + icp_solve_deferred_kernel under MISLAM_ICP_FUSED_SOLVE=0 MISLAM_ICP_TICKET_SOLVE=0.
Error-sum producers (mi_icp_run, read before relied upon):
  sync_every = 1: every iteration is followed by icp_flush_pending -- K4/K5 on the fused path, then icp_rows_reduce + icp_finalize_pending;
  carried: the fused search of iteration k + 1 carries iteration k's error, and the state keeps those sums only if the solve behind it fires
    a stop rule.  A run capped at max_iterations = k is NOT enqueued past the cap (batch_len in mi_icp_run), so its last error comes from
    the flush again; the carried sums are reached with max_iterations = -1, eps a hair above iteration k's error (taken from the stepped
    run, whose earlier errors are asserted to lie above it), sync_every = k + 2 and a budget of k + 1 iterations: STOP_CONVERGED at k.
mi_icp_result does not report the pair count of a registration; `pairs == mom[0]` is asserted where it is reported (mi_kabsch).
icp_batch.hip exposes no sums: it stays covered by its bit equality with the single call (tests/test_gpu_icp_batch.py).

Solve: T_k against compose(T_(k-1), solve(the device's own moments)) within icp_sums_reference.solve_bars, wherever the float64 solve is
well-posed (kabsch_catalogue.WELL_POSED; every size from 5 points on is asserted to be)."""
import os
import re

import numpy as np
import pytest

import icp_sums_reference as S
from conftest import ROOT, check_measured

pytestmark = pytest.mark.gpu


def _header(name):
    return open(os.path.join(ROOT, "cuda-slam_amd", "csrc", name)).read()


def _constexpr(header, name):
    return int(re.search(r"constexpr int %s = (\d+);" % name, _header(header)).group(1))


MAX_ROWS = _constexpr("kernels.h", "ICP_FUSED_SOLVE_MAX_ROWS")
REDUCED = _constexpr("kernels.h", "ICP_REDUCED_ROWS")
CHUNK = _constexpr("kernels.h", "ICP_CHUNK_POINTS")
HELPER_FULL_MAX = _constexpr("nn_grid.h", "GRID_HELPER_FULL_MAX_POINTS")
COLD_PASSES = int(re.search(r"#define MISLAM_GRID_COLD_PASSES (\d+)", _header("nn_grid.h")).group(1))
WARM = COLD_PASSES + 1                                     # the first iteration whose search is the warm kernel (extend_reach off)

SWITCHES = {"default": {}, "counting": {}, "onewave": {"MISLAM_GRID_SPLIT_WALKS": "0"}, "ticket_small": {"MISLAM_ICP_FUSED_SOLVE": "0"},
            "two_launch": {"MISLAM_ICP_FUSED_SOLVE": "0", "MISLAM_ICP_TICKET_SOLVE": "0"}}
# producer -> (context, nn_mode, the search kernel's name, fused)
PRODUCERS = {"helper": ("default", "NN_GRID", "nn_grid_kernel", True), "onewave": ("onewave", "NN_GRID", "nn_grid_kernel", True),
             "counting": ("counting", "NN_GRID", "nn_grid_kernel", True), "brute": ("default", "NN_BRUTEFORCE", "nn_bruteforce_kernel", False),
             "tree": ("default", "NN_TREE", "nn_tree_kernel", False), "world1": ("world1", "NN_GRID", "nn_grid_kernel", True)}
FUSED = tuple(p for p, v in PRODUCERS.items() if v[3])
# (dist_mode, compose_mode, filter_pairs) by position in SIZES: both values of each rule at small, ragged and large sizes
RULES = ((0, 0, 1), (1, 1, 0), (0, 1, 1), (1, 0, 1), (0, 0, 0), (1, 1, 1), (0, 1, 0), (1, 0, 0), (0, 0, 1), (1, 1, 1), (0, 1, 0), (1, 0, 1))


def test_sizes_exercise_what_they_are_named_for():
    assert (MAX_ROWS, REDUCED, CHUNK) == (S.FUSED_SOLVE_MAX_ROWS, S.REDUCED_ROWS, S.ROW_POINTS)        # the reference counts with the kernels' constants
    assert S.STRIPS == 1024 // (16 + 2) == 56
    assert S.SIZES[-3:] == (CHUNK * MAX_ROWS, S.N_THRESHOLD, S.N_RAGGED) and len(RULES) == len(S.SIZES)
    assert S.row_count(CHUNK * MAX_ROWS) == MAX_ROWS and S.row_count(S.N_THRESHOLD) == MAX_ROWS + 1       # the last one-workgroup size, the first beyond
    r = S.row_count(S.N_RAGGED)
    assert r > MAX_ROWS and r % S.reduced_count(r) != 0 and S.N_RAGGED % CHUNK != 0
    assert [n % 4 for n in (1, 2, 3, 5)] == [1, 2, 3, 1] and 63 % CHUNK and 65 % CHUNK and 255 % CHUNK      # partly filled quads and rows
    assert S.row_count(4097) == 65 == CHUNK + 1 and S.reduced_count(65) == 3                              # one row past a wave of rows; ragged slices
    assert max(S.SIZES) <= HELPER_FULL_MAX                                                                # every default fused search has its helper wave
    assert WARM == 7 and {r[0] for r in RULES} == {r[1] for r in RULES} == {r[2] for r in RULES} == {0, 1}
    assert S.M_FIXED < 10000                                                                              # (NN_AUTO would not index it: the modes are forced)


@pytest.fixture(scope="module")
def ctxs(capi):
    """Contexts by name, created on first use under their developer switches (read once, at context creation)."""
    made = {}

    def get(name):
        if name not in made:
            if name == "world1":
                made[name] = capi.Context(0, 0, 1, capi.dist_unique_id())
                assert made[name].rank_world() == (0, 1)
            else:
                saved = {k: os.environ.get(k) for k in SWITCHES[name]}
                os.environ.update(SWITCHES[name])
                try:
                    made[name] = capi.Context(0)
                finally:
                    for k, v in saved.items():
                        if v is None:
                            os.environ.pop(k, None)
                        else:
                            os.environ[k] = v
                if name == "counting":
                    made[name].search_stats(True)
        return made[name]
    yield get
    for c in made.values():
        c.close()


_clouds = {}


def clouds(n):
    if n not in _clouds:
        _clouds[n] = S.clouds(n)
    return _clouds[n]


def reducer_of(ctx_name, n):
    if ctx_name in ("world1", "two_launch"):
        return ctx_name
    return "ticket" if ctx_name == "ticket_small" or S.row_count(n) > MAX_ROWS else "one_workgroup"


def check_reducer(sched, fused, route, n, k):
    """The schedule read-back behind iteration k tells the reducers apart."""
    nrows = S.row_count(n)
    assert sched["ticket"] == 0 and len(sched["order"]) == nrows
    if not fused or route == "one_workgroup":
        assert not sched["cursors"].any() and np.array_equal(sched["order"], np.arange(nrows)), (route, n, k)       # no work order is dealt
    elif route == "ticket":
        pair = 2 * ((k - 1) & 1)
        assert sched["cursors"][pair] + sched["cursors"][pair + 1] == nrows and not sched["cursors"][2 - pair:4 - pair].any(), (n, k, sched["cursors"])
        assert np.array_equal(np.sort(sched["order"]), np.arange(nrows))
    else:
        assert not sched["cursors"].any() and np.array_equal(np.sort(sched["order"]), np.arange(nrows)), (route, n, k)


class Steps:
    """A registration stepped one iteration at a time (sync_every = 1: every iteration's error through icp_flush_pending)."""

    def __init__(self, capi, ctxs, search, producer, n, rules, iterations, ctx_name=None, max_d2=None):
        self.capi, self.search, self.producer, self.n, self.rules = capi, search, producer, n, rules
        self.ctx_name, mode, kernel, self.fused = PRODUCERS[producer]
        self.ctx_name = ctx_name or self.ctx_name
        self.c = c = ctxs(self.ctx_name)
        self.before, self.after = clouds(n)
        self.dist, self.compose, self.filter = rules
        self.nn_mode = getattr(capi, mode)
        assert c.nn_kernel_name(n, len(self.after), self.nn_mode) == kernel
        self.identity = (np.eye(3, dtype=np.float32), np.zeros(3, np.float32))
        self.pairs = {}
        idx, d2 = self.matches(1)
        self.max_d2 = S.median_filter(d2) if max_d2 is None else max_d2
        self.params = dict(dist_mode=self.dist, compose_mode=self.compose, filter_pairs=self.filter, max_distance_squared=self.max_d2,
                           nn_mode=self.nn_mode, abort_on_increase=0)
        self.mom_route = reducer_of(self.ctx_name, n)
        self.flush_route = "world1" if self.ctx_name == "world1" else "two_launch"        # icp_rows_reduce + icp_finalize_pending (+ the all-reduce)
        if self.ctx_name == "counting":
            c.search_stats(True)
        c.icp_load(self.before, self.after, capi.icp_params(eps=0.0, max_iterations=-1, sync_every=1, **self.params))
        self.out = []
        for k in range(1, iterations + 1):
            done = c.icp_run(1)
            R, t, it, err, why = c.icp_result()
            sched = c.selftest_icp_schedule()
            self.out.append(dict(R=R, t=t, it=it, err=np.float32(err), why=why, sums=sched["sums"].copy(), sched=sched))
            if why != capi.STOP_RUNNING:
                break
            assert done == 1 and it == k, (producer, n, k, done, it, why)
            check_reducer(sched, self.fused, self.mom_route, n, k)
        if self.ctx_name == "counting":                     # the counting build ran: it counted every point of every search
            assert c.search_stats(True)[3] == n * len(self.out), (n, len(self.out))

    def pose(self, k):
        return self.identity if k == 0 else (self.out[k - 1]["R"], self.out[k - 1]["t"])

    def matches(self, k):
        """The pairs of iteration k: the every-pair search of the cloud moved by T_(k-1)."""
        if k not in self.pairs:
            cur = S.transform(self.before, *self.pose(k - 1))
            idx, d2 = self.search.nn_search(cur, self.after, self.dist, self.capi.NN_BRUTEFORCE)
            self.pairs[k] = (cur, idx, d2)
        return self.pairs[k][1:]

    def use(self, k):
        idx, d2 = self.matches(k)
        return d2 < np.float32(self.max_d2) if self.filter else np.ones(self.n, bool)

    def check_sums(self, k, sums, what, route, worst, tag):
        """what: "mom" or "err" -- the device's sums of iteration k against the reference inside the route's bounds."""
        idx, _ = self.matches(k)
        use, matched = self.use(k), self.after[idx]
        if what == "mom":
            ref, mag = S.moments(self.pairs[k][0], matched, use)
            got = sums[:16]
        else:
            ref, mag = S.error_sums(matched, S.transform(self.before, *self.pose(k)), use)
            got = sums[16:]
        bound = S.bounds(self.n, route, mag)
        ratio = 0.0
        for c in range(len(ref)):
            diff = float(abs(np.longdouble(got[c]) - ref[c]))
            if bound[c] == 0.0:
                assert np.longdouble(got[c]) == ref[c], (tag, self.n, k, what, c, got[c], float(ref[c]))        # the counts, and sums of zeros: exact
            else:
                assert diff <= bound[c], (tag, self.n, k, what, c, got[c], float(ref[c]), diff, bound[c])
                ratio = max(ratio, diff / bound[c])
        print("%s n=%d k=%d %s (%s, k=%d additions): kept %d of %d, worst |diff| / bound %.3f" % (tag, self.n, k, what, route, S.additions(self.n, route), int(use.sum()), self.n, ratio))
        worst["sums"] = max(worst.get("sums", 0.0), ratio)
        return use

    def check_error_value(self, k, err, sums):
        denom = sums[17] if self.filter else float(len(self.after))                      # finalize_iteration's rule
        want = np.float32(sums[16] / denom)
        assert np.float32(err).tobytes() == want.tobytes(), (self.producer, self.n, k, err, want)

    def check_solve(self, k, worst, tag):
        o = self.out[k - 1]
        R_prev, t_prev = self.pose(k - 1)
        sol = S.solve(o["sums"][:16])
        if not sol["well"]:
            assert self.n < 5 or o["sums"][0] < 4, (tag, self.n, k, sol["cond"])          # only a handful of pairs leave the rotation undetermined
            return
        R_ref, t_ref = S.compose(R_prev, t_prev, sol["R"], sol["t"], self.compose)
        bar_r, bar_t = S.solve_bars(sol, t_prev, self.compose)
        d_r, d_t = float(np.abs(o["R"] - R_ref).max()), float(np.abs(o["t"] - t_ref).max())
        print("%s n=%d k=%d solve: |dR| %.3e (bar %.3e) |dt| %.3e (bar %.3e) cond %.2e" % (tag, self.n, k, d_r, bar_r, d_t, bar_t, sol["cond"]))
        assert d_r <= bar_r and d_t <= bar_t, (tag, self.n, k, d_r, bar_r, d_t, bar_t)
        worst["solve"] = max(worst.get("solve", 0.0), d_r / bar_r, d_t / bar_t)

    def check(self, k, worst, tag=None):
        tag = tag or self.producer
        o = self.out[k - 1]
        assert o["why"] == self.capi.STOP_RUNNING and np.isfinite(o["sums"]).all(), (tag, self.n, k, o["why"])
        use = self.check_sums(k, o["sums"], "mom", self.mom_route, worst, tag)
        self.check_sums(k, o["sums"], "err", self.flush_route, worst, tag)
        if self.filter and self.n >= 63:
            assert 0.2 * self.n < use.sum() < 0.8 * self.n, (tag, self.n, k, int(use.sum()))      # about half the lanes drop out
        self.check_error_value(k, o["err"], o["sums"])
        self.check_solve(k, worst, tag)

    def carried(self, k, worst):
        """Iteration k's error sums as the fused search of iteration k + 1 carries them (module docstring), through the moments' reducer."""
        capi, c = self.capi, self.c
        errs = [o["err"] for o in self.out[:k]]
        eps = np.nextafter(errs[-1], np.float32(np.inf))
        assert all(e >= eps for e in errs[:-1]), (self.producer, self.n, k, errs)           # the rule cannot fire before iteration k
        c.icp_load(self.before, self.after, capi.icp_params(eps=float(eps), max_iterations=-1, sync_every=k + 2, **self.params))
        c.icp_run(k + 1)
        R, t, it, err, why = c.icp_result()
        sums = c.selftest_icp_schedule()["sums"]
        o = self.out[k - 1]
        assert why == capi.STOP_CONVERGED and it == k - 1, (self.producer, self.n, k, why, it)
        assert R.tobytes() == o["R"].tobytes() and t.tobytes() == o["t"].tobytes()           # the same registration: T_k
        assert sums[:16].tobytes() == o["sums"][:16].tobytes()                               # iteration k + 1's moments were not applied
        self.check_sums(k, sums, "err", self.mom_route, worst, self.producer + "/carried")
        self.check_error_value(k, err, sums)


def record(key, worst):
    check_measured("icp_sums_ratio_%s" % key, worst.get("sums", 0.0), 1.0, floor=0.05)
    if "solve" in worst:
        check_measured("icp_sums_solve_ratio_%s" % key, worst["solve"], 1.0, floor=0.05)


@pytest.mark.parametrize("producer", list(PRODUCERS))
def test_sums_at_every_size(capi, ctxs, ctx, producer):
    """Iterations 1 (no previous match, identity pose) and 2 at every size, largest first; the rules change with the size."""
    worst = {}
    for n, rules in reversed(list(zip(S.SIZES, RULES))):
        run = Steps(capi, ctxs, ctx, producer, n, rules, 2)
        for k in (1, 2):
            run.check(k, worst)
    record(producer, worst)


@pytest.mark.parametrize("ctx_name", ["ticket_small", "two_launch"])
@pytest.mark.parametrize("producer", ["helper", "brute"])
def test_sums_through_the_other_reducers(capi, ctxs, ctx, producer, ctx_name):
    """The ticket form below its size, the two launches at every size: fused and unfused rows."""
    worst = {}
    for n in (S.N_RAGGED, S.N_THRESHOLD, CHUNK * MAX_ROWS, 4097, 65, 5, 1):
        run = Steps(capi, ctxs, ctx, producer, n, (n & 1, (n >> 1) & 1, 1), 2, ctx_name=ctx_name)
        assert run.mom_route == ("ticket" if ctx_name == "ticket_small" else "two_launch")
        for k in (1, 2):
            run.check(k, worst, tag="%s/%s" % (producer, ctx_name))
    record("%s_%s" % (producer, ctx_name), worst)


@pytest.mark.parametrize("filter_pairs", [0, 1])
@pytest.mark.parametrize("compose", [0, 1])
@pytest.mark.parametrize("dist", [0, 1])
def test_every_rule_on_fused_and_unfused_rows(capi, ctxs, ctx, dist, compose, filter_pairs):
    worst = {}
    for producer in ("helper", "brute"):
        for n in (4097, 255):
            run = Steps(capi, ctxs, ctx, producer, n, (dist, compose, filter_pairs), 3)
            for k in (1, 2, 3):
                run.check(k, worst)
    record("rules_%d%d%d" % (dist, compose, filter_pairs), worst)


@pytest.mark.parametrize("producer", list(PRODUCERS))
def test_warm_iterations(capi, ctxs, ctx, producer):
    """Up to the first iteration behind the cold passes: warm starts from the previous matches, a non-identity fp32 pose, the warm search
    kernel (extend_reach off); every iteration at 4 097 points, the second and the last beyond the one-workgroup size."""
    worst = {}
    for n, ks, rules in ((S.N_THRESHOLD, (2, WARM), (0, 1, 1)), (4097, range(1, WARM + 1), (1, 0, 1))):
        run = Steps(capi, ctxs, ctx, producer, n, rules, WARM)
        assert len(run.out) == WARM
        for k in ks:
            run.check(k, worst)
    record("warm_%s" % producer, worst)


@pytest.mark.parametrize("producer", FUSED)
def test_error_sums_carried_by_the_next_search(capi, ctxs, ctx, producer):
    worst = {}
    # (an unfiltered registration under the exact composition lowers its error with every iteration: the warm iteration is reached there;
    # the filter and cpu-slam's additive translation ride at the first two iterations -- carried() asserts what it relies on)
    for n, rules, ks in ((S.N_RAGGED, (0, 1, 0), (1, 2, WARM)), (4097, (1, 1, 1), (1, 2)), (4097, (1, 1, 0), (WARM,)), (65, (0, 0, 1), (1, 2))):
        run = Steps(capi, ctxs, ctx, producer, n, rules, max(ks))
        for k in ks:
            run.carried(k, worst)
    record("carried_%s" % producer, worst)


@pytest.mark.parametrize("producer,ctx_name", [("helper", None), ("onewave", None), ("brute", None), ("tree", None), ("world1", None),
                                               ("helper", "two_launch"), ("brute", "ticket_small")])
def test_every_pair_dropped(capi, ctxs, ctx, producer, ctx_name):
    """max_distance_squared = 0 under filter_pairs: no lane has a pair.  All 18 sums are exactly zero -- behind a registration that left the
    rows full -- and the registration stops for want of pairs."""
    for n in (S.N_THRESHOLD, 4097, 65):
        Steps(capi, ctxs, ctx, producer, n, (0, 0, 1), 2, ctx_name=ctx_name)                 # rows full of other sums
        run = Steps(capi, ctxs, ctx, producer, n, (0, 0, 1), 1, ctx_name=ctx_name, max_d2=0.0)
        o = run.out[0]
        assert o["why"] == capi.STOP_NO_PAIRS and o["it"] == 0, (producer, n, o["why"])
        assert (o["sums"] == 0.0).all(), (producer, n, o["sums"])
        assert np.array_equal(o["R"], np.eye(3, dtype=np.float32)) and not o["t"].any()


def test_stand_alone_sums(capi, ctx):
    """mi_cross_moments, mi_kabsch and mi_transform_mse on the caller's pairs with half of them masked out: K2 / K4+K5, icp_rows_reduce,
    the butterfly -- the two-launch count.  mi_transform_mse returns the mean as a float: it must be the rounding of a quotient inside
    the sum's bound (rounding is monotone: the interval's ends are rounded)."""
    worst = {}
    rng = np.random.default_rng(5)
    R, t = S.rotation(0.1).astype(np.float32), np.array([0.3, -0.2, 0.25], np.float32)
    for n in reversed(S.SIZES):
        before, after = clouds(n)
        idx = rng.integers(0, len(after), n).astype(np.int32)
        keep = (rng.uniform(size=n) < 0.5).astype(np.uint8)
        keep[rng.integers(0, n)] = 1
        use = keep > 0
        ref, mag = S.moments(before, after[idx], use)
        bound = S.bounds(n, "two_launch", mag)
        got = ctx.cross_moments(before, after, idx, keep)
        diff = np.abs(got.astype(np.longdouble) - ref).astype(np.float64)
        assert got[0] == ref[0] and (diff <= bound).all(), (n, diff, bound)
        worst["sums"] = max(worst.get("sums", 0.0), float((diff[1:] / bound[1:]).max()))
        assert ctx.kabsch(before, after, idx, keep)[2] == int(got[0])                        # pairs == mom[0]
        out, mse = ctx.transform_mse(before, R, t, after, idx, keep, divide_by_pairs=True)
        new = S.transform(before, R, t)
        assert out.tobytes() == new.tobytes()
        err, emag = S.error_sums(after[idx], new, use)
        d = S.bounds(n, "two_launch", emag)[0] / float(err[1]) + 2.0 ** -52 * float(err[0] / err[1])      # the sum's bound, the fp64 division's rounding
        q = float(err[0] / err[1])
        print("stand-alone n=%d: moments worst %.3f of the bound; mse %.9g in [%.9g, %.9g]" % (n, float((diff[1:] / bound[1:]).max()), mse, np.float32(q - d), np.float32(q + d)))
        assert np.float32(q - d) <= np.float32(mse) <= np.float32(q + d), (n, mse, q, d)
    record("stand_alone", worst)


def test_lane_layout_exactly(ctx):
    """Pairwise distinct small integer coordinates: every product and every sum of them is exact in fp64 and every squared error in fp32, so
    the expected sums hold with == for ANY mask.  One-hot masks for each of the 64 lanes of the first row and of a row in the middle: each
    moment is the single pair's product, e0 its fp32 value -- a lane mapped to the wrong column, or lost, shows.  Then one kept lane per
    quad at each quad position, a different position in every quad, and ragged prefixes."""
    n, m = 5 * 64 + 7, 301
    rng = np.random.default_rng(11)
    before = rng.permutation(np.arange(1, 1500))[:3 * n].reshape(n, 3).astype(np.float32)
    after = rng.permutation(np.arange(1, 1500))[:3 * m].reshape(m, 3).astype(np.float32)
    idx = rng.integers(0, m, n).astype(np.int32)
    T = S.pair_terms(before, after[idx])
    eye, zero = np.eye(3, dtype=np.float32), np.zeros(3, np.float32)
    e = S.pair_errors(after[idx], before)
    assert (e == ((after[idx].astype(np.float64) - before) ** 2).sum(axis=1)).all() and e.max() < 2 ** 24      # exact in fp32

    def check(keep, tag):
        use = keep > 0
        got = ctx.cross_moments(before, after, idx, keep)
        assert np.array_equal(got, T[use].sum(axis=0)), (tag, got, T[use].sum(axis=0))
        _, mse = ctx.transform_mse(before, eye, zero, after, idx, keep, divide_by_pairs=True, want_cloud=False)
        assert np.float32(mse) == np.float32(e[use].astype(np.float64).sum() / use.sum()), (tag, mse)

    for row in (0, 2):
        for lane in range(64):
            keep = np.zeros(n, np.uint8)
            keep[64 * row + lane] = 1
            check(keep, ("one-hot", row, lane))
    lanes = np.arange(n) % 64
    for q in range(4):
        check((lanes % 4 == q).astype(np.uint8), ("quad position", q))
        check((lanes % 4 == (lanes // 4 + q) % 4).astype(np.uint8), ("rotating quad position", q))
    for count in (1, 2, 3, 5, 63, 65, n - 1, n):
        check((np.arange(n) < count).astype(np.uint8), ("prefix", count))
