"""GPU suite: the non-iterative registration (K10, csrc/nicp_api.hip) stage by stage against tests/nicp_reference.py, the float64 restatement
tests/test_nicp_reference.py pins against the oracle.  tests/test_gpu_nicp.py sees the final pick of whole runs; here every stage is held to
a bound that follows from its arithmetic:

  a. the 32 raw sums (Context.selftest_nicp_candidates): within (max(m, n) + 8) 2^-53 sum|term| of moments(); the spare entry exactly 0
  b. a candidate's rotation: D = U_a^T R U_b with the axes of the centred float64 Gram matrices; the signs of diag(D) are the oracle's on the
     same permuted clouds, | |D| - I | <= max(2 x the oracle's own deviation on the case, 16 * 2^-23 / relative gap).  The oracle's deviation,
     measured on these cases: 2e-7 .. 1.1e-6 up to 2500 points, 2e-6 .. 2.5e-5 at 131 073 (fp32 QR over N points); the gap term is 5e-6 .. 3e-5
  c. its translation: |t - (ca - R cb)| <= 2^-23 max(1, |t|) + 1e-12 max|c| with the device's own R
  d. its approximated error: within 2^-23 approx + (m + 8) 2^-53 (Saa + tr Gb + 2 |Sab|_1) / m of approx_error() with the device's own R
  e. b - d again on a cloud 1e5 units out along (1, 1, 1): the host's formula in float64 holds the bounds at every offset up to there once
     the sums are taken about the clouds' first points (tests/test_nicp_reference.py; raw coordinates miss bound d from 1e3 on)
  f. the exact error of one candidate: out_T has the selftest candidate's bits, the error is within 2^-23 of exact_error() on it, the nearest
     neighbours behind it are the restatement's; subclouds of 1, 63, 64, 65 points and the whole cloud; the box-hierarchy route once
  g. the pick over 9 repetitions in the three modes: driver() on the device's approximated errors and the restatement's exact errors of the
     device's candidates gives the registration's repetition count and winner; a tie, an overflowing list, an early exit.  No case is left out
  h. no subcloud point within the limit: MI_OK, the first candidate scored, FLT_MAX, max_repetitions
  i. hygiene: repeatable bits, other calls in between, no ICP problem stays loaded, no buffer outlives its context, refusals write nothing"""
import ctypes as C

import numpy as np
import pytest

import nicp_reference as N

pytestmark = pytest.mark.gpu

# one point past what the moments kernel's grid covers in ONE trip of its grid-stride loop: icp_reduce_blocks caps the grid at 512 workgroups of
# 256 threads, so at 131 073 points thread 0 takes a second point and everything else does not
BEYOND_ONE_PASS = N.ONE_PASS + 1
SIZES = [(k, k) for k in (4, 5, 63, 64, 65, 257, 2500)] + [(63, 65), (64, 257), (1000, 2500), (257, 64), (BEYOND_ONE_PASS, BEYOND_ONE_PASS)]
KINDS = ("rigid", "noisy", "loose")
FAR = np.full(3, 1e5)                    # e: the largest offset of tests/test_nicp_reference.py's table
MIN_GAP = 0.05


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32).tolist()


def make_cloud(kind, m, n, shift):
    """The first seed from a fixed start whose two clouds have well separated axes (relative gaps >= 0.06): small samples of an anisotropic
    Gaussian do not all have them."""
    for seed in range(m * 7 + n, m * 7 + n + 200):
        b, a = N.loose_pair(seed, m, n, shift) if kind == "loose" else N.rigid_pair(seed, m, n, 0.0 if kind == "rigid" else 0.01, shift)
        if N.min_gap(b, a) >= 0.06:
            return b, a
    raise AssertionError("no seed with separated axes")


def make_heads(m, n, reps):
    rng = np.random.default_rng(m + 3 * n)
    return np.stack([np.arange(3)] + [rng.permutation(min(m, n))[:3] for _ in range(reps - 1)]).astype(np.int32)


def check_candidates(oracle, b, a, heads, raw, R, t, approx, label, oracle_about_first=False):
    """oracle_about_first: the oracle is handed the clouds taken about their first points (exact in fp32 for the cloud 1e5 out, whose points
    are multiples of 2^-7): its fp32 centroid of raw coordinates of that size is off by half a unit and its axes with it, while the signs it is
    asked for do not depend on where the clouds lie."""
    m, n = len(b), len(a)
    # a
    ref, mag = N.moments(b, a)
    bound = (max(m, n) + 8) * N.U64 * np.asarray(mag, np.float64)
    err = np.abs(np.asarray(np.asarray(raw, np.longdouble) - ref, np.float64))
    print("%s: raw sums worst error / bound %.3f" % (label, float((err / np.maximum(bound, 1e-300)).max())))
    assert (err <= bound).all(), (np.nonzero(err > bound)[0].tolist(), err, bound)
    assert raw[31] == 0.0
    # b
    c = N.centred(b, a)
    (Ub, _, gb), (Ua, _, ga) = N.axes(c["Gb"]), N.axes(c["Ga"])
    gap = float(min(gb.min(), ga.min()))
    assert gap >= MIN_GAP
    Ds, Do = [], []
    for k, head in enumerate(heads):
        pb, pa = N.permuted(b, a, N.full_permutation(head, min(m, n)))
        if oracle_about_first:
            assert (pb - b[0]).astype(np.float64).tolist() == (pb.astype(np.float64) - b[0]).tolist()
            assert (pa - a[0]).astype(np.float64).tolist() == (pa.astype(np.float64) - a[0]).tolist()
            pb, pa = pb - b[0], pa - a[0]
        Ro = oracle.nicp_single(pb, pa)[0]
        Do.append(Ua.T @ Ro.astype(np.float64) @ Ub)
        Ds.append(Ua.T @ R[k].astype(np.float64) @ Ub)
    dev_o = max(np.abs(np.abs(D) - np.eye(3)).max() for D in Do)
    dev = max(np.abs(np.abs(D) - np.eye(3)).max() for D in Ds)
    allowed = max(2.0 * dev_o, 16 * N.EPS32 / gap)
    print("%s: gap %.3f, | |D| - I | device %.2e oracle %.2e allowed %.2e" % (label, gap, dev, dev_o, allowed))
    assert dev <= allowed
    for D, O in zip(Ds, Do):
        assert np.array_equal(np.sign(np.diag(D)), np.sign(np.diag(O)))
    # c, d
    floor = N.approx_floor(c)
    cmax = max(np.abs(c["ca"]).max(), np.abs(c["cb"]).max())
    for k in range(len(heads)):
        t_ref = c["ca"] - R[k].astype(np.float64) @ c["cb"]
        assert (np.abs(t[k] - t_ref) <= N.EPS32 * np.maximum(1.0, np.abs(t[k])) + 1e-12 * cmax).all(), (k, t[k], t_ref)
        if m > n:                  # the pair sums lack sum b over the pairs alone: no approximated error there, and no mode that reads one
            continue
        e_ref = N.approx_error(R[k], b, a)
        print("%s: rep %d approx %.9e reference %.9e, 2^-23 approx %.2e + floor %.2e" % (label, k, approx[k], e_ref, N.EPS32 * e_ref, floor))
        assert abs(float(approx[k]) - e_ref) <= N.EPS32 * e_ref + floor, (k, approx[k], e_ref)


@pytest.mark.parametrize("where", ["origin", "shifted"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("m,n", SIZES)
def test_sums_and_candidates(ctx, oracle, m, n, kind, where):
    b, a = make_cloud(kind, m, n, N.SHIFT if where == "shifted" else None)
    heads = make_heads(m, n, 4 if m < 10000 else 2)
    raw, R, t, approx = ctx.selftest_nicp_candidates(b, a, heads)
    check_candidates(oracle, b, a, heads, raw, R, t, approx, "%d x %d %s %s" % (m, n, kind, where))


@pytest.mark.parametrize("kind", ["rigid", "noisy"])
def test_far_from_the_origin(ctx, oracle, kind):
    b, a = N.rigid_pair(17507, 2500, 2500, 0.0 if kind == "rigid" else 0.01, FAR)
    heads = make_heads(2500, 2500, 4)
    raw, R, t, approx = ctx.selftest_nicp_candidates(b, a, heads)
    check_candidates(oracle, b, a, heads, raw, R, t, approx, "2500 x 2500 %s at 1e5" % kind, oracle_about_first=True)


# ---- f. the exact error of one candidate ----
def register(ctx, capi, b, a, heads, sub, mode, eps):
    p = capi.nicp_params(eps=eps, max_repetitions=len(heads), approximation=mode)
    return ctx.nicp_register(b, a, p, heads, sub)


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("sub_n", [1, 63, 64, 65, None])
@pytest.mark.parametrize("where", ["origin", "shifted"])
def test_exact_error_of_one_candidate(ctx, capi, where, sub_n, mode):
    m, n = 257, 300
    b, a = make_cloud("noisy", m, n, N.SHIFT if where == "shifted" else None)
    head = make_heads(m, n, 3)[2:3]
    sub = None if sub_n is None else np.random.default_rng(sub_n).permutation(m)[:sub_n].astype(np.int32)
    _, Rc, tc, _ = ctx.selftest_nicp_candidates(b, a, head)
    R, t, reps, err = register(ctx, capi, b, a, head, sub, mode, 1e-9)
    assert reps == 1 and bits(R) == bits(Rc[0]) and bits(t) == bits(tc[0])
    pts = b if sub is None else b[sub]
    mean, kept, idx, d2 = N.exact_error(R, t, pts, a)
    print("sub %s mode %d %s: error %.9e restatement %.9e kept %d" % (sub_n, mode, where, err, mean, kept))
    assert kept == len(pts) and abs(float(err) - mean) <= N.EPS32 * mean
    kidx, kd2 = ctx.knn_search(N.transform(R, t, pts), a, 1)
    assert np.array_equal(kidx[:, 0], idx) and bits(kd2[:, 0]) == bits(d2)


def test_exact_error_through_the_box_hierarchy(ctx, capi):
    # 63 246^2 >= 4e9 pairs: the registration scores through the search's own choice of kernel (MI_NN_AUTO), not the every-pair one
    n = 63246
    assert float(n) * n >= 4e9 > float(n - 1) * (n - 1)
    b, a = make_cloud("noisy", n, n, None)
    head = make_heads(n, n, 2)[1:2]
    _, Rc, tc, _ = ctx.selftest_nicp_candidates(b, a, head)
    R, t, reps, err = register(ctx, capi, b, a, head, None, 0, 1e-12)
    assert reps == 1 and bits(R) == bits(Rc[0]) and bits(t) == bits(tc[0])
    kidx, kd2 = ctx.knn_search(N.transform(R, t, b), a, 1)
    d2 = kd2[:, 0].astype(np.float64)
    mean = float(np.sum(d2[d2 < 1e6].astype(np.longdouble)) / (d2 < 1e6).sum())
    assert (d2 < 1e6).all() and abs(float(err) - mean) <= N.EPS32 * mean


# ---- g. the pick ----
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("eps", [1e-9, 1e-3])
@pytest.mark.parametrize("order", ["falling", "mixed"])
@pytest.mark.parametrize("m,n", [(257, 257), (1000, 2500)])
def test_the_pick_is_the_restated_drivers(ctx, capi, m, n, order, eps, mode):
    b, a, heads, sub = N.pick_case(m, n, order)
    _, Rc, tc, approx = ctx.selftest_nicp_candidates(b, a, heads)
    labels = [bytes(np.concatenate([Rc[k].ravel(), tc[k]]).tobytes()) for k in range(9)]
    exact = [N.exact_error(Rc[k], tc[k], b[sub], a)[0] for k in range(9)]
    assert len(set(labels)) == 8 and labels[PICK_TIE[order][0]] == labels[PICK_TIE[order][1]]        # two equal heads, one candidate
    assert len(set(approx.tolist())) >= 7
    assert N.near_ties(exact, labels) == [] and all(abs(e - eps) > 2.0 ** -20 * eps for e in exact)   # no case needs leaving out
    d = N.driver(list(range(9)), approx, [np.float32(e) for e in exact], eps, mode)
    R, t, reps, err = register(ctx, capi, b, a, heads, sub, mode, eps)
    assert reps == d["repetitions"]
    assert np.concatenate([R.ravel(), t]).astype(np.float32).tobytes() == labels[d["winner"]]
    assert abs(float(err) - exact[d["winner"]]) <= N.EPS32 * exact[d["winner"]]
    if mode == 2 and order == "falling":
        assert d["overflowed"] and len(d["listed"]) == 5
    if mode == 0 and order == "mixed" and eps == 1e-3 and m == n:
        assert reps == 5


PICK_TIE = {"falling": (3, 4), "mixed": (2, 3)}


# ---- h. nothing within the limit ----
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_no_point_within_the_limit(ctx, capi, mode):
    b = np.array([[0.0, 0.0, 0.0], [1.0, 0.1, 0.0], [0.2, 0.6, 0.1], [0.1, 0.3, 0.4]], np.float32)
    a = (3000.0 * np.array([[1.0, 0.0, 0.0], [-1.0, 0.2, 0.0], [0.0, -1.0, 0.3], [0.1, 0.8, -1.2]])).astype(np.float32)
    heads = np.array([[0, 1, 2], [3, 1, 0], [2, 3, 1]], np.int32)
    _, Rc, tc, approx = ctx.selftest_nicp_candidates(b, a, heads)
    for k in range(3):
        assert N.exact_error(Rc[k], tc[k], b, a)[1] == 0                                # every nearest d2 >= 1e6 on the restatement
    d = N.driver([0, 1, 2], approx, [np.nan] * 3, 1e-3, mode)
    R, t, reps, err = register(ctx, capi, b, a, heads, None, mode, 1e-3)
    assert reps == 3 and np.float32(err) == N.FLT_MAX
    assert bits(R) == bits(Rc[d["winner"]]) and bits(t) == bits(tc[d["winner"]])
    assert d["winner"] == (0 if mode == 0 else d["listed"][0])
    assert abs(abs(np.linalg.det(R.astype(np.float64))) - 1.0) <= 1e-5


# ---- i. hygiene ----
def test_same_bits_again_and_after_other_calls(ctx, capi, bunny):
    b, a = make_cloud("noisy", 1000, 2500, N.SHIFT)
    heads = make_heads(1000, 2500, 4)

    def run():
        raw, R, t, approx = ctx.selftest_nicp_candidates(b, a, heads)
        return raw.view(np.uint64).tolist(), bits(R), bits(t), bits(approx)

    first = run()
    assert run() == first
    normals = ctx.estimate_normals(a, 8)
    ctx.knn_search(None, a, 8)
    ctx.fpfh_features(a, normals, 8)
    ctx.icp_register(bunny[0][:2000], bunny[1][:2000], capi.icp_params(max_iterations=3))
    assert run() == first


def test_no_icp_problem_stays_loaded(ctx, capi, bunny):
    # the selftest uploads into the buffers a loaded problem lives in: like mi_nicp_register it leaves no problem loaded behind it
    b, a = make_cloud("noisy", 64, 64, None)
    ctx.icp_load(bunny[0][:2000], bunny[1][:2000], capi.icp_params(max_iterations=5))
    ctx.icp_run(2)
    ctx.selftest_nicp_candidates(b, a, make_heads(64, 64, 2))
    with pytest.raises(capi.MiSlamError):
        ctx.icp_run(2)
    ctx.icp_load(bunny[0][:2000], bunny[1][:2000], capi.icp_params(max_iterations=5))
    ctx.icp_run(2)
    ctx.nicp_register(b, a, capi.nicp_params(max_repetitions=2, approximation=0), make_heads(64, 64, 2), None)
    with pytest.raises(capi.MiSlamError):
        ctx.icp_run(2)


def test_no_buffer_outlives_its_context(capi):
    b, a = make_cloud("noisy", 257, 300, None)
    start = capi.selftest_live_buffers()
    with capi.Context(0) as own:
        own.selftest_nicp_candidates(b, a, make_heads(257, 300, 3))
        assert capi.selftest_live_buffers() > start
    assert capi.selftest_live_buffers() - start == 0


def test_refusals_leave_the_outputs_untouched(ctx, capi):
    b, a = make_cloud("noisy", 64, 65, None)
    heads = make_heads(64, 65, 2)
    f = capi.lib().mi_selftest_nicp_candidates
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    f.restype = C.c_int
    raw, out = np.full(32, 7.0), np.full((2, 13), 7.0, np.float32)

    def call(before=b, m=64, after=a, n=65, h=heads, reps=2, r=raw, o=out, handle=ctx._h):
        ptr = lambda x: None if x is None else x.ctypes.data
        return f(handle, ptr(before), m, ptr(after), n, ptr(h), reps, ptr(r), ptr(o))

    bad = heads.copy()
    bad[1, 2] = 64                                                   # min(m, n) = 64: one past the last pair
    low = heads.copy()
    low[0, 0] = -1
    refused = [dict(m=2), dict(n=2), dict(h=bad), dict(h=low), dict(reps=-1), dict(before=None), dict(after=None), dict(h=None), dict(r=None),
               dict(o=None), dict(handle=None)]
    for kw in refused:
        assert call(**kw) == capi.MI_ERR_INVALID_ARG, kw
        assert (raw == 7.0).all() and (out == 7.0).all(), kw
    assert call() == 0 and raw[31] == 0.0 and not (out == 7.0).any()
