"""GPU suite: the 19 M-step moments of every CPD route, the solve that reads them, the transform behind it and the exact sigma^2_0, each
against the float64 reference of tests/mstep_reference.py.

Every case runs whole EM iterations through cpd_register (or one cpd_mstep) and reads back what the call left on the device
(Context.selftest_cpd_last): the arrays of the LAST E-step, the moments the last solve read, the state, the transformed cloud.  A moment is
compared with the float64 sum over the arrays the same launch produced, so the E-step's own tolerance never enters.

Routes and their producers of the moments (asserted from the read-back's route / rows / fused / reduced entries -- a case that falls through
to another route fails -- and once more from the profile counters, test_profile_counters_agree_with_the_routes):
  exact_mfma, exact_valu   cpd_post_den_kernel / cpd_post_contract_kernel: 64 points per row, at most 512 rows
  every_pair               the same post kernels behind the every-pair truncated E-step (MISLAM_CPD_TRUNC_CULL=0, hybrid mode)
  sequential               MI_ESTEP_CPU_SEQUENTIAL: the stand-alone cpd_xsums_kernel / cpd_ksums_kernel, 256 points per row, at most 512 rows
  culled                   cpd_trunc_den_kernel / cpd_trunc_contract_kernel: curve-ordered tiles of 64, at most 4096 rows
  fgt                      fgt_post_kt1_kernel / fgt_post_px_kernel: 256 points per row, at most 512 rows
  world1                   a distributed context of one rank: the post kernels, cpd_reduce_sums_kernel, the solve from the state block
  mstep                    mi_cpd_mstep on the caller's arrays: the stand-alone sums
The hybrid mode takes the truncated E-step only once sigma^2 <= 0.015 sigma^2_0, and a registration's sigma^2_0 is its first sigma^2: the
truncated routes therefore run one FGT iteration from a large sigma^2_0 first (constant scale: the cloud keeps its size) and are read back
after the truncated iteration(s) behind it; the moving cloud and sigma^2 that E-step started from come from the same registration stopped an
iteration earlier (the library is deterministic to the bit).

Bounds (mstep_reference.moment_bounds -- derived from the producers' arithmetic, nothing measured):
  Every term of a moment is a product of two float32 values formed in fp64 -- exact -- so the only error is that of the fp64 additions:
  |device - reference| <= gamma_k sum|term|, k = the longest chain of additions a term goes through on that producer:
    a lane adds one term per grid-stride trip, ceil(ceil(points / per_row) / rows) trips (1 below the row cap, 2 just past it);
    + 6 levels of the wave's shuffle tree; + 3 for the four waves of a workgroup (none on the truncated kernels, whose sums stay on wave 0);
    + the one-workgroup sum of the rows: 256 / W row groups (W = 8 x-sums, 16 k-sums) of ceil(rows / groups) rows each, then the groups.
  No producer keeps part of a sum in fp32.  xs[4] and ks[13] round a_d a_d / b_d b_d to float32 before the exact product with the weight
  (+ 2^-24 sum|term|) and add the three products first (k + 2).  A moment whose terms are all zero must be exactly zero.
  L = -xs[0] + 1.5 n log sigma^2 against reference A of tests/estep_reference.py / tests/fgt_reference.py with their L bound and their bar.
  Solve: R 1e-5, t 1e-4, scale 1e-4 relative (tests/test_gpu_cpd.py) against mstep_reference.solve on the device's own moments; sigma^2
  absolutely within mstep_reference.sigma2_bound (c = 1640 fp32 roundings on the cancelling terms, counted there).
  Transform: bit for bit.  sigma^2_0: mstep_reference.sigma2_init_bound (fp64 sums, the closed form's cancellation, one narrowing)."""
import math
import os

import numpy as np
import pytest

import estep_reference as ER
import fgt_reference as FR
import mstep_reference as M
from conftest import check_measured

pytestmark = pytest.mark.gpu

ROUTES = ("exact_mfma", "exact_valu", "sequential", "culled", "every_pair", "fgt", "world1", "mstep")
PRODUCER = {"exact_mfma": "post", "exact_valu": "post", "every_pair": "post", "world1": "post", "sequential": "standalone",
            "mstep": "standalone", "fgt": "standalone", "culled": "trunc"}
CONTEXT = {"exact_valu": "valu", "every_pair": "nocull", "world1": "world1"}
ROW_EDGE = {"post": (32768, 32769), "standalone": (131072, 131073), "trunc": (262144, 262145)}
SIZES = (4097, 257, 256, 255, 65, 64, 63, 2, 1)            # descending: on a shared context a row count that is too large reads a stale row
FAR = 1.0e4                                                  # moving points this far out: every affinity underflows / lies beyond the truncation
L_MAX_PAIRS = 3_000_000                                      # the dense float64 E-step reference stays below a second


@pytest.fixture(scope="module")
def ctxs(capi):
    """Contexts by name, created on first use under their developer switch (read once, at context creation)."""
    switches = {"default": None, "valu": ("MISLAM_CPD_MFMA", "0"), "nocull": ("MISLAM_CPD_TRUNC_CULL", "0"), "ieee": ("MISLAM_SVD_IEEE", "1")}
    made = {}

    def get(name):
        if name not in made:
            if name == "world1":
                made[name] = capi.Context(0, 0, 1, capi.dist_unique_id())
            else:
                sw = switches[name]
                old = os.environ.get(sw[0]) if sw else None
                if sw:
                    os.environ[sw[0]] = sw[1]
                try:
                    made[name] = capi.Context(0)
                finally:
                    if sw:
                        if old is None:
                            del os.environ[sw[0]]
                        else:
                            os.environ[sw[0]] = old
        return made[name]
    yield get
    for c in made.values():
        c.close()


def rotation(angle=0.2):
    axis = np.array([1.0, 2.0, 3.0]) / math.sqrt(14.0)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * (K @ K)


def clouds(m, n, seed, half=5.0, offset=(0.0, 0.0, 0.0), far=0):
    """Moving cloud uniform in a cube of half-width `half` about `offset`; the fixed cloud: points of it rotated by 0.2 rad about the cube's
    centre with noise of 3 % of the width.  far: that many moving points (among them the last one) moved FAR away."""
    rng = np.random.default_rng(seed)
    b = rng.uniform(-half, half, (m, 3))
    a = b[rng.integers(0, m, n)] @ rotation().T + rng.normal(scale=0.06 * half, size=(n, 3))
    off = np.asarray(offset, np.float64)
    b, a = (b + off).astype(np.float32), (a + off).astype(np.float32)
    rows = np.array([], np.int64)
    if far:
        rows = np.unique(np.concatenate([[m - 1], rng.integers(0, m, far - 1)]))
        b[rows] += np.float32(FAR)
    return b, a, rows


def spread(b, a, far_rows):
    """(trace of the live moving cloud's covariance + the fixed cloud's) / 3: the sigma^2 a constant-scale M-step lands on from a diffuse P."""
    live = np.delete(b.astype(np.float64), far_rows, axis=0)
    return float((live.var(axis=0).sum() + a.astype(np.float64).var(axis=0).sum()) / 3.0)


class Run:
    """One registration (or M-step) on a route and what it left behind."""

    def __init__(self, capi, ctxs, route, b, a, sigma2, far_rows=(), iters=1, const_scale=0, ctx_name=None, arrays_from=None):
        self.route, self.b, self.a, self.const_scale, self.iters = route, b, a, const_scale, iters
        m, n = len(b), len(a)
        self.ctx = ctx = ctxs(ctx_name or CONTEXT.get(route, "default"))
        self.estep_y, self.estep_sigma2 = b, np.float32(sigma2)       # what the read-back E-step started from
        common = dict(eps=0.0, tolerance=0.0, const_scale=const_scale)
        if route == "mstep":
            src = arrays_from
            ctx.cpd_mstep(b, a, src["p1"], src["pt1"], src["px"], const_scale, 1.0, float(sigma2))
            self.rb = ctx.selftest_cpd_last(m, n)
            want_route, self.truncated = -1, False
        elif route in ("culled", "every_pair"):
            # iteration 1: FGT from sigma^2_0 = 100 x the spread; iterations 2 .. 1 + iters: truncated (sigma^2 <= 0.015 sigma^2_0 from there on)
            s0 = 100.0 * spread(b, a, far_rows)
            p = dict(common, const_scale=1, approximation=capi.CPD_APPROX_HYBRID, sigma2_init=s0)
            self.const_scale = 1
            ctx.cpd_register(b, a, capi.cpd_params(max_iterations=iters, **p))
            before = ctx.selftest_cpd_last(m, n)
            assert before["iterations"] == iters and before["route"] == (capi.CPD_ROUTE_FGT if iters == 1 else self.trunc_route(capi))
            assert float(before["sigma2"]) <= 0.015 * float(before["sigma2_init"]), (before["sigma2"], before["sigma2_init"])
            self.estep_y, self.estep_sigma2 = before["y"], before["sigma2"]
            ctx.cpd_register(b, a, capi.cpd_params(max_iterations=iters + 1, **p))
            self.rb = ctx.selftest_cpd_last(m, n)
            want_route, self.truncated = self.trunc_route(capi), True
            self.iters = iters + 1
        else:
            p = dict(common, sigma2_init=float(sigma2))
            if route == "sequential":
                p["estep_mode"] = capi.ESTEP_CPU_SEQUENTIAL
            if route == "fgt":
                p["approximation"] = capi.CPD_APPROX_FULL
            if iters > 1:                                   # the E-step read back is the last one: its inputs from the run stopped before it
                ctx.cpd_register(b, a, capi.cpd_params(max_iterations=iters - 1, **p))
                before = ctx.selftest_cpd_last(m, n)
                self.estep_y, self.estep_sigma2 = before["y"], before["sigma2"]
            ctx.cpd_register(b, a, capi.cpd_params(max_iterations=iters, **p))
            self.rb = ctx.selftest_cpd_last(m, n)
            want_route = {"exact_mfma": capi.CPD_ROUTE_EXACT_MFMA, "world1": capi.CPD_ROUTE_EXACT_MFMA, "exact_valu": capi.CPD_ROUTE_EXACT_VALU,
                          "sequential": capi.CPD_ROUTE_SEQUENTIAL, "fgt": capi.CPD_ROUTE_FGT}[route]
            self.truncated = False
        rb = self.rb
        # the intended route ran, with the rows its producer leaves
        prod = PRODUCER[route]
        fused = 0 if route in ("sequential", "mstep") else 1
        assert rb["route"] == want_route, (route, rb["route"])
        assert (rb["fused"], rb["rows_x"], rb["rows_k"]) == (fused, M.sum_rows(n, prod), M.sum_rows(m, prod)), (route, m, n, rb["fused"], rb["rows_x"], rb["rows_k"])
        assert rb["reduced"] == (1 if route == "world1" else 0)
        if route == "world1":
            assert ctx.rank_world() == (0, 1)
        if route != "mstep":
            assert rb["iterations"] == self.iters, (route, rb["iterations"], rb["stop_reason"])

    def trunc_route(self, capi):
        return capi.CPD_ROUTE_TRUNC_CULLED if self.route == "culled" else capi.CPD_ROUTE_TRUNC_EVERY_PAIR

    # ---- check 1: the 18 array-determined moments
    def moments_ratio(self):
        rb, m, n = self.rb, len(self.b), len(self.a)
        for k in ("p1", "pt1", "px"):
            assert np.isfinite(rb[k]).all(), (self.route, m, n, k)
        xs, ks, xs_abs, ks_abs = M.moments(self.b, self.a, rb["p1"], rb["pt1"], rb["px"])
        bx, bk = M.moment_bounds(m, n, PRODUCER[self.route], xs_abs, ks_abs)
        worst = 0.0
        for name, got, ref, bound, idx in (("xs", rb["xs"], xs, bx, M.XS_ARRAY_SUMS), ("ks", rb["ks"], ks, bk, M.KS_SUMS)):
            for i in idx:
                err = abs(float(got[i]) - float(ref[i]))
                print("moment %s %dx%d %s[%d]: device %.17g reference %.17g |diff| %.3e bound %.3e" % (self.route, m, n, name, i, got[i], ref[i], err, bound[i]))
                if bound[i] == 0.0:
                    assert got[i] == 0.0, (self.route, m, n, name, i, got[i])
                    continue
                assert err <= bound[i], (self.route, m, n, name, i, float(got[i]), float(ref[i]), err, float(bound[i]))
                worst = max(worst, err / bound[i])
        return worst

    # ---- check 2: xs[0] through L, against the float64 E-step references and their own bound and bar
    def L_ratio(self, oracle):
        rb, m, n = self.rb, len(self.b), len(self.a)
        if self.route == "mstep" or m * n > L_MAX_PAIRS:
            return None
        s2 = float(np.float32(self.estep_sigma2))
        L = -float(rb["xs"][0]) + 1.5 * n * math.log(s2)
        out = (rb["p1"], rb["pt1"], rb["px"], L)
        if self.route == "fgt":
            case = FR.Case("moments", "moments", self.estep_y, self.a, s2, 0.3, 8, 10.0, float(rb["sigma2_init"]))
            r = FR.references(case, kcenter=oracle.fgt_kcenter, ck=oracle.fgt_ck, with_b=False)["A"]
            ratio, bar = FR.ratios(out, r)["L"][0], FR.BAR
        else:
            case = ER.Case("moments", "moments", self.estep_y, self.a, s2, 0.3)
            case.constant = float(rb["constant"])
            mode = "trunc" if self.truncated else "exact"
            path = {"exact_mfma": "mfma", "world1": "mfma", "exact_valu": "valu", "sequential": "oracle", "culled": "culled", "every_pair": "every_pair"}[self.route]
            r = ER.references(case, modes=(mode,))[mode]["A"]
            ratio, bar = ER.ratios(out, r, path)["L"][0], ER.BAR
        print("L %s %dx%d: device %.9g ratio %.3f of its bound (bar %g)" % (self.route, m, n, L, ratio, bar))
        assert ratio <= bar, (self.route, m, n, L, ratio)
        return ratio / bar

    # ---- check 5: the transform, bit for bit
    def check_transform(self):
        rb = self.rb
        if self.route == "mstep":                          # (an M-step alone transforms nothing: the cloud as loaded)
            assert np.array_equal(rb["y"], self.b)
            return
        want = M.transform(self.b, rb["R"], rb["t"], rb["scale"])
        same = rb["y"].view(np.uint32) == want.view(np.uint32)
        assert same[-1].all(), (self.route, len(self.b), rb["y"][-1], want[-1])              # the last live point
        assert same.all(), (self.route, len(self.b), int((~same).sum()), np.argwhere(~same)[:4].tolist())

    # ---- check 3: the solve, against the float64 solve of the device's own moments (or of `moments`: check 4)
    def solve_ratio(self, moments=None):
        rb = self.rb
        xs, ks = (rb["xs"], rb["ks"]) if moments is None else moments
        sol = M.solve(xs, ks, self.const_scale, 1.0)
        # the bars hold for clouds centred at the origin: the centring terms stay below the moments they are subtracted from
        assert sol["Np"] * float(sol["ca"] @ sol["ca"]) <= abs(sol["sigmaSubtrahend"]) and sol["Np"] * float(sol["cb"] @ sol["cb"]) <= abs(sol["scaleDenominator"])
        dR = float(np.abs(rb["R"].astype(np.float64) - sol["R"]).max())
        dt = float(np.abs(rb["t"].astype(np.float64) - sol["t"]).max())
        ds = abs(float(rb["scale"]) - sol["scale"]) / abs(sol["scale"])
        d2 = abs(float(rb["sigma2"]) - sol["sigma2"])
        b2 = M.sigma2_bound(sol, self.const_scale)
        print("solve %s %dx%d cs=%d: |dR| %.3e |dt| %.3e dscale %.3e |dsigma2| %.3e (bound %.3e, sigma2 %.6g)" % (self.route, len(self.b), len(self.a), self.const_scale, dR, dt, ds, d2, b2, sol["sigma2"]))
        assert dR <= 1e-5 and dt <= 1e-4 and ds <= 1e-4 and d2 <= b2, (self.route, dR, dt, ds, d2, b2)
        return max(dR / 1e-5, dt / 1e-4, ds / 1e-4, d2 / b2)


def run_case(capi, ctxs, oracle, route, b, a, sigma2, worst, arrays_ctx="default", **kw):
    """A case on a route: the moments, L, the transform.  The mstep route is fed the arrays an exact run on the same clouds left."""
    if route == "mstep":
        src = Run(capi, ctxs, "exact_mfma", b, a, sigma2, **{k: v for k, v in kw.items() if k != "iters"}).rb
        run = Run(capi, ctxs, "mstep", b, a, sigma2, arrays_from=src, **{k: v for k, v in kw.items() if k != "iters"})
    else:
        run = Run(capi, ctxs, route, b, a, sigma2, **kw)
    worst["moments"] = max(worst.get("moments", 0.0), run.moments_ratio())
    lr = run.L_ratio(oracle)
    if lr is not None:
        worst["L"] = max(worst.get("L", 0.0), lr)
    run.check_transform()
    return run


def record(route, worst):
    check_measured("cpd_moments_ratio_%s" % route, worst.get("moments", 0.0), 1.0, floor=0.05)
    if "L" in worst:
        check_measured("cpd_moments_L_ratio_%s" % route, worst["L"], 1.0, floor=0.05)


def min_points(route):
    return 2 if route in ("fgt", "culled", "every_pair") else 1          # the FGT (and the hybrid mode's first iteration) needs two points per side


@pytest.mark.parametrize("side", ["moving", "fixed"])
@pytest.mark.parametrize("route", ROUTES)
def test_moments_at_the_ragged_sizes(capi, ctxs, oracle, route, side):
    """1 .. 4097 points on one side, 65 or 257 on the other (m != n), largest first on the route's context."""
    worst = {}
    for size in SIZES:
        if size < min_points(route):
            continue
        other = 65 if size == 257 else 257 if size in (65, 4097) else 65
        m, n = (size, other) if side == "moving" else (other, size)
        b, a, _ = clouds(m, n, seed=1000 + size)
        run_case(capi, ctxs, oracle, route, b, a, 1.0, worst)
    record(route, worst)


@pytest.mark.parametrize("side", ["moving", "fixed"])
@pytest.mark.parametrize("route", ROUTES)
def test_moments_at_the_row_cap(capi, ctxs, oracle, route, side):
    """The last size that fills the producer's rows one trip deep and the first that wraps into a second trip; then a small problem on the
    same context, whose rows sit in front of the stale ones."""
    worst = {}
    for size in reversed(ROW_EDGE[PRODUCER[route]]):
        m, n = (size, 65) if side == "moving" else (65, size)
        b, a, _ = clouds(m, n, seed=size)
        run_case(capi, ctxs, oracle, route, b, a, 1.0, worst)
    b, a, _ = clouds(65, 63, seed=7)
    run_case(capi, ctxs, oracle, route, b, a, 1.0, worst)
    record(route, worst)


@pytest.mark.parametrize("route", ROUTES)
def test_moments_of_an_offset_cloud(capi, ctxs, oracle, route):
    """Extent 1 at (100, -50, 30): the moments are fp64 and hold their bound (the solve's fp32 centring is the reference's own: not checked)."""
    worst = {}
    b, a, _ = clouds(300, 257, seed=31, half=0.5, offset=(100.0, -50.0, 30.0))
    run_case(capi, ctxs, oracle, route, b, a, 0.1, worst)
    record(route, worst)


@pytest.mark.parametrize("route", ROUTES)
def test_rows_with_zero_p1_contribute_nothing(capi, ctxs, oracle, route):
    worst = {}
    b, a, far = clouds(321, 257, seed=57, far=40)
    run = run_case(capi, ctxs, oracle, route, b, a, 1.0, worst, far_rows=far)
    assert (run.rb["p1"][far] == 0).all() and (run.rb["px"][far] == 0).all()
    live = np.setdiff1d(np.arange(len(b)), far)
    assert (run.rb["p1"][live] != 0).all()
    # the reference over the live rows alone is the reference over all of them: the device's moments are within the live rows' bound of it
    xs, ks, xs_abs, ks_abs = M.moments(b[live], a, run.rb["p1"][live], run.rb["pt1"], run.rb["px"][live])
    bx, bk = M.moment_bounds(len(b), len(a), PRODUCER[route], xs_abs, ks_abs)
    assert (np.abs(run.rb["ks"] - ks) <= bk).all(), (route, np.abs(run.rb["ks"] - ks), bk)
    record(route, worst)


@pytest.mark.parametrize("route", ["exact_mfma", "culled"])
def test_moments_after_two_consecutive_iterations(capi, ctxs, oracle, route):
    """The identities against the arrays of the second (truncated route: the second truncated) E-step; nothing of the first may be left in the rows."""
    worst = {}
    b, a, _ = clouds(1000, 900, seed=77)
    run = run_case(capi, ctxs, oracle, route, b, a, 1.0, worst, iters=2)
    assert run.rb["iterations"] == (3 if route == "culled" else 2)
    record(route + "_two_iterations", worst)


SOLVE_ROUTES = ("exact_mfma", "exact_valu", "sequential", "fgt", "world1", "mstep")


@pytest.mark.parametrize("ctx_name", ["default", "ieee"])
@pytest.mark.parametrize("const_scale", [0, 1])
def test_solve_matches_the_float64_solve_of_its_own_moments(capi, ctxs, oracle, const_scale, ctx_name):
    """Clouds centred at the origin, 10 units across (the bunny's extent): fast and IEEE 3 x 3 SVD, both scale rules, ragged sizes."""
    worst = 0.0
    for m, n, seed in ((1000, 900, 1), (257, 4097, 2), (4097, 300, 3)):
        b, a, _ = clouds(m, n, seed=seed)
        for route in ("exact_mfma", "mstep"):
            if route == "mstep":
                src = Run(capi, ctxs, "exact_mfma", b, a, 1.0, const_scale=const_scale, ctx_name=ctx_name).rb
                run = Run(capi, ctxs, "mstep", b, a, 1.0, const_scale=const_scale, ctx_name=ctx_name, arrays_from=src)
            else:
                run = Run(capi, ctxs, route, b, a, 1.0, const_scale=const_scale, ctx_name=ctx_name)
            worst = max(worst, run.solve_ratio())
            run.check_transform()
    check_measured("cpd_solve_ratio_%s_cs%d" % (ctx_name, const_scale), worst, 1.0, floor=0.05)


@pytest.mark.parametrize("route,const_scale", [(r, cs) for r in ROUTES for cs in (0, 1) if cs or r not in ("culled", "every_pair")])
def test_solve_is_independent_of_the_route(capi, ctxs, oracle, route, const_scale):
    """All routes end in the one solve: the route's own transform, and mi_cpd_mstep's from the arrays the route left, lie within the bars of the
    SAME float64 solve (of the float64 moments of those arrays).  (The truncated routes are reached behind a constant-scale FGT iteration:
    constant scale only.)"""
    b, a, _ = clouds(1000, 900, seed=5)
    if route == "mstep":
        first = Run(capi, ctxs, "exact_mfma", b, a, 1.0, const_scale=const_scale)
    else:
        first = Run(capi, ctxs, route, b, a, 1.0, const_scale=const_scale)
    arrays = first.rb
    xs, ks, _, _ = M.moments(b, a, arrays["p1"], arrays["pt1"], arrays["px"])
    xs[0] = 0.0
    second = Run(capi, ctxs, "mstep", b, a, 1.0, const_scale=first.const_scale, arrays_from=arrays)
    if first.route in ("culled", "every_pair"):
        # (the state's scale going into a constant-scale M-step is the registration's: 1)
        assert float(first.rb["scale"]) == 1.0
    worst = max(first.solve_ratio((xs, ks)), second.solve_ratio((xs, ks)))
    check_measured("cpd_solve_route_ratio_%s_cs%d" % (route, const_scale), worst, 1.0, floor=0.05)


def test_exact_sigma2_init(capi, ctxs):
    """cpd_sigma_squared (exact mode) against the centred float64 sums: ragged sizes, the 131 072 / 131 073 edge of cpd_init_sums' rows on
    either side, the offset cloud."""
    ctx = ctxs("default")
    worst = 0.0
    cases = [clouds(131073, 65, 1)[:2], clouds(65, 131073, 2)[:2], clouds(131072, 257, 3)[:2], clouds(257, 131072, 4)[:2]]
    cases += [clouds(m, n, 10 + m)[:2] for m, n in ((4097, 257), (257, 65), (65, 257), (63, 64), (2, 65), (1, 2), (1, 1), (255, 256))]
    cases += [clouds(300, 257, 31, half=0.5, offset=(100.0, -50.0, 30.0))[:2], clouds(131073, 300, 32, half=0.5, offset=(100.0, -50.0, 30.0))[:2]]
    for b, a in cases:
        got, ref, bound = ctx.cpd_sigma_squared(b, a), M.sigma2_exact(b, a), M.sigma2_init_bound(b, a)
        err = abs(got - ref) / ref
        print("sigma2_0 %dx%d: device %.9g reference %.9g rel %.3e bound %.3e" % (len(b), len(a), got, ref, err, bound))
        assert err <= bound, (len(b), len(a), got, ref, err, bound)
        worst = max(worst, err / bound)
    check_measured("cpd_sigma2_init_ratio", worst, 1.0, floor=0.05)


def test_profile_counters_agree_with_the_routes(capi, ctxs):
    """The same route decisions seen from the per-kernel launch counters: the FGT E-step under its own counter, the sequential parity mode
    under the denominators' alone, the exact and the truncated E-steps under both."""
    b, a, _ = clouds(300, 257, seed=3)
    for route in ("exact_mfma", "sequential", "fgt", "culled", "every_pair"):
        ctx = ctxs(CONTEXT.get(route, "default"))
        ctx.profile_enable(True)
        try:
            ctx.profile_reset()
            run = Run(capi, ctxs, route, b, a, 1.0)              # (asserts the read-back's route)
            n = {k: ctx.profile_get(k)[1] for k in (capi.KERNEL_CPD_DENOM, capi.KERNEL_CPD_CONTRACT, capi.KERNEL_CPD_FGT, capi.KERNEL_CPD_MSTEP)}
        finally:
            ctx.profile_enable(False)
        den, con, fgt, mst = n[capi.KERNEL_CPD_DENOM], n[capi.KERNEL_CPD_CONTRACT], n[capi.KERNEL_CPD_FGT], n[capi.KERNEL_CPD_MSTEP]
        # (an exact registration enqueues its iterations in batches: those behind the stopping one return at once but are counted)
        if route == "exact_mfma":
            assert den >= 1 and con == den and fgt == 0 and mst >= 1, (route, n)
        elif route == "sequential":
            assert den >= 1 and con == 0 and fgt == 0 and mst >= 1, (route, n)
        elif route == "fgt":
            assert (den, con, fgt, mst) == (0, 0, 1, 1), (route, n)
        else:                                                   # an FGT iteration, then a truncated one -- in each of the two registrations of the Run
            assert (den, con, fgt, mst) == (1, 1, 2, 3), (route, n)
        assert run.rb["iterations"] == run.iters


def test_read_back_refuses_what_it_cannot_vouch_for(capi, ctxs):
    ctx = ctxs("default")
    b, a, _ = clouds(65, 63, seed=1)
    ctx.cpd_register(b, a, capi.cpd_params(max_iterations=1, sigma2_init=1.0))
    with pytest.raises(capi.MiSlamError):
        ctx.selftest_cpd_last(64, 63)                            # not the loaded sizes
    first = ctx.selftest_cpd_last(65, 63)
    again = ctx.selftest_cpd_last(65, 63, arrays=False)          # repeatable, every array optional
    assert np.array_equal(first["ks"], again["ks"]) and "p1" not in again
    ctx.cpd_sigma_squared(b, a)                                  # another entry point has used the workspace since
    with pytest.raises(capi.MiSlamError):
        ctx.selftest_cpd_last(65, 63)
    with capi.Context(0) as fresh:
        with pytest.raises(capi.MiSlamError):
            fresh.selftest_cpd_last(65, 63)                      # no CPD call at all
