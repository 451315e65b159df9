"""GPU suite: mi_segment_plane and mi_segment_plane_hypotheses against the numpy restatement of their contract (tests/segment_reference.py).
Triples, flags, counts, winners and labels are integers and are compared for equality; a plane may differ from the restatement's by one
float32 unit in the last place per component (the device's fp64 root and division may differ from numpy's in the last fp64 bit, which can
move the float32 rounding by one step at most), and every count and label is then held to a float64 recount under the DEVICE's plane.
Not covered: the refusal of a distributed context (MI_ERR_STATE) -- no GPU test of this tree shows a cheap way to an exchange context."""
import ctypes as C
import functools

import numpy as np
import pytest

import segment_reference as R
from conftest import synth_cloud
from test_segment_abi import axis_case, planted_three

pytestmark = pytest.mark.gpu

THR, H, SEED = 0.05, 600, 1


def ulps(a, b):
    """distance in float32 units in the last place, per component"""
    def key(v):
        i = np.ascontiguousarray(v, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(2 ** 31) - i, i)
    return np.abs(key(a) - key(b))


def tilted_planes(sizes, clutter, thr, seed):
    """points on tilted planes through a box of 10 with Gaussian noise of a quarter of thr along the normal, uniform clutter, permuted"""
    rng = np.random.default_rng(seed)
    normals = np.array([[0.3, -0.5, 0.8], [0.7, 0.6, -0.4], [-0.6, 0.35, 0.7]])
    parts = []
    for k, size in enumerate(sizes):
        nrm = normals[k] / np.linalg.norm(normals[k])
        u = np.cross(nrm, [1.0, 0.0, 0.0])
        u /= np.linalg.norm(u)
        v = np.cross(nrm, u)
        st = rng.uniform(-5, 5, (size, 2))
        parts.append(st[:, :1] * u + st[:, 1:] * v + (1.5 * k - 1.0) * nrm + 0.25 * thr * rng.normal(size=(size, 1)) * nrm)
    parts.append(rng.uniform(-5, 5, (clutter, 3)))
    cloud = np.concatenate(parts).astype(np.float32)
    cloud = cloud[rng.permutation(len(cloud))]
    cloud.setflags(write=False)
    return cloud


@functools.lru_cache(maxsize=None)
def scene():
    return tilted_planes((3000, 2000, 1000), 1000, THR, 2026)


@functools.lru_cache(maxsize=None)
def scene_ref(refine):
    return R.segment(scene(), THR, H, SEED, refine, max_planes=4, min_inliers=300)


@functools.lru_cache(maxsize=None)
def scene_hyp():
    return R.hypotheses(scene(), np.arange(len(scene())), SEED, 0, H)


def call(ctx, cloud, thr, **kw):
    planes, inliers, labels, rmse, winners = ctx.segment_plane(cloud, thr, want_labels=True, want_rmse=True, want_winners=True, **kw)
    return dict(planes=planes, inliers=inliers, labels=labels, rmse=rmse, winners=winners, n_planes=len(planes))


def recount(cloud, dev, thr):
    """what the device's own planes give in float64, round by round: labels, counts, and rmse within one ulp; |(a, b, c)| = 1 within 2^-23"""
    labels = np.full(len(cloud), -1, np.int32)
    for p in range(dev["n_planes"]):
        index = np.flatnonzero(labels < 0)
        mask = R.inlier_mask(dev["planes"][p], cloud[index], thr)[0]
        assert int(mask.sum()) == dev["inliers"][p] >= 3, (p, int(mask.sum()), dev["inliers"][p])
        assert ulps(dev["rmse"][p], R.rmse_of(dev["planes"][p], cloud[index], mask)) <= 1, p
        P = dev["planes"][p].astype(np.float64)
        assert abs(np.sqrt((P[0] * P[0] + P[1] * P[1]) + P[2] * P[2]) - 1.0) <= 2.0 ** -23, p
        labels[index[mask]] = p
    assert np.array_equal(labels, dev["labels"])
    return True


def same_as_reference(dev, ref):
    assert dev["n_planes"] == ref["n_planes"] and np.array_equal(dev["winners"], ref["winners"])
    assert np.array_equal(dev["planes"].view(np.uint32), ref["planes"].view(np.uint32))
    assert np.array_equal(dev["inliers"], ref["inliers"]) and np.array_equal(dev["labels"], ref["labels"])
    assert np.array_equal(dev["rmse"].view(np.uint32), ref["rmse"].view(np.uint32)) or (ulps(dev["rmse"], ref["rmse"]) <= 1).all()
    return True


def check_unrefined(ctx, cloud, thr, **kw):
    """refine_iterations = 0: equal to the restatement wherever the device's planes are bit-equal to its; a plane one ulp off is held to the
    recount under the device's planes alone (and ends the comparison of the later rounds, whose points may differ)"""
    dev, ref = call(ctx, cloud, thr, refine_iterations=0, **kw), R.segment(cloud, thr, refine_iterations=0, **{"hypotheses_per_plane" if k == "hypotheses" else k: v for k, v in kw.items()})
    if dev["n_planes"]:
        recount(cloud, dev, thr)
    if dev["n_planes"] == ref["n_planes"] and np.array_equal(dev["planes"].view(np.uint32), ref["planes"].view(np.uint32)):
        return same_as_reference(dev, ref), dev
    p = next(p for p in range(min(dev["n_planes"], ref["n_planes"]) + 1)
             if p >= min(dev["n_planes"], ref["n_planes"]) or not np.array_equal(dev["planes"][p].view(np.uint32), ref["planes"][p].view(np.uint32)))
    assert p < min(dev["n_planes"], ref["n_planes"]) and dev["winners"][p] == ref["winners"][p] and (ulps(dev["planes"][p], ref["planes"][p]) <= 1).all(), p
    assert np.array_equal(dev["winners"][:p], ref["winners"][:p]) and np.array_equal(dev["inliers"][:p], ref["inliers"][:p])
    return False, dev


def test_the_restatement_alone_finds_the_three_planes():
    for refine in (0, 1, 2):
        ref = scene_ref(refine)
        assert ref["n_planes"] == 3 and (np.diff(ref["inliers"]) < 0).all()
        for got, planted in zip(ref["inliers"], (3000, 2000, 1000)):
            assert planted * 0.95 <= got <= planted + 100
    _, valid, _ = scene_hyp()
    assert valid.sum() >= H - 5


def test_hypotheses_against_the_restatement(ctx):
    cloud = scene()
    triples, valid, plane4, count = ctx.segment_plane_hypotheses(cloud, THR, H, SEED)
    rt, rv, rp = scene_hyp()
    assert np.array_equal(triples, rt) and np.array_equal(valid.astype(bool), rv)
    assert (ulps(plane4, rp) <= 1).all() and (plane4[~rv] == 0).all()
    print("planes bit-equal to the restatement: %d of %d" % ((ulps(plane4, rp).max(axis=1) == 0).sum(), H))
    assert np.array_equal(count, R.counts(plane4, rv, cloud, THR))                # equal to a float64 recount under the device's own plane
    w = ctx.segment_plane_hypotheses(cloud, THR, H, SEED, first=100, count=57)    # a window
    for got, whole in zip(w, (triples, valid, plane4, count)):
        assert np.array_equal(got, whole[100:157])


def test_unrefined_call_equals_the_restatement(ctx):
    exact, dev = check_unrefined(ctx, scene(), THR, hypotheses=H, seed=SEED, max_planes=4, min_inliers=300)
    assert exact and same_as_reference(dev, scene_ref(0))


def test_one_refinement_step_against_eigh(ctx):
    cloud = scene()
    dev = call(ctx, cloud, THR, hypotheses=H, seed=SEED, refine_iterations=1, max_planes=1, min_inliers=300)
    assert dev["n_planes"] == 1 and recount(cloud, dev, THR)
    h = int(dev["winners"][0])
    _, _, plane4, _ = ctx.segment_plane_hypotheses(cloud, THR, H, SEED, first=h, count=1)
    mask = R.inlier_mask(plane4[0], cloud, THR)[0]
    assert (ulps(dev["planes"][0], R.refit(cloud, mask, plane4[0])) <= 1).all()


def test_two_refinement_steps(ctx):
    cloud = scene()
    dev, ref = call(ctx, cloud, THR, hypotheses=H, seed=SEED, refine_iterations=2, max_planes=4, min_inliers=300), scene_ref(2)
    assert dev["n_planes"] == ref["n_planes"] == 3 and recount(cloud, dev, THR)
    assert (dev["inliers"] >= 3).all() and np.abs(dev["planes"].astype(np.float64) - ref["planes"]).max() <= 1e-5


def small_cloud(n, seed):
    return tilted_planes((n - n // 4,), n // 4, THR, seed)


@pytest.mark.parametrize("n", [257, 513])
def test_a_tile_plus_one(ctx, n):
    cloud = small_cloud(n, n)
    triples, valid, plane4, count = ctx.segment_plane_hypotheses(cloud, THR, 300, 5)
    rt, rv, rp = R.hypotheses(cloud, np.arange(n), 5, 0, 300)
    assert np.array_equal(triples, rt) and np.array_equal(valid.astype(bool), rv) and (ulps(plane4, rp) <= 1).all()
    assert np.array_equal(count, R.counts(plane4, rv, cloud, THR))
    check_unrefined(ctx, cloud, THR, hypotheses=300, seed=5, max_planes=2, min_inliers=20)
    assert recount(cloud, call(ctx, cloud, THR, hypotheses=300, seed=5, refine_iterations=2, max_planes=2, min_inliers=20), THR)


@pytest.mark.parametrize("hyp", [1, 255, 257])
def test_hypothesis_counts_around_a_workgroup(ctx, hyp):
    cloud = small_cloud(1000, 77)
    triples, valid, plane4, count = ctx.segment_plane_hypotheses(cloud, THR, hyp, 3)
    rt, rv, rp = R.hypotheses(cloud, np.arange(1000), 3, 0, hyp)
    assert np.array_equal(triples, rt) and np.array_equal(valid.astype(bool), rv) and (ulps(plane4, rp) <= 1).all()
    assert np.array_equal(count, R.counts(plane4, rv, cloud, THR))
    check_unrefined(ctx, cloud, THR, hypotheses=hyp, seed=3, max_planes=1, min_inliers=3)


def test_three_points_and_one_hypothesis(ctx):
    cloud = np.array([[0, 0, 0], [1, 0, 0.5], [0, 2, 0.25]], np.float32)
    seed = next(s for s in range(100) if len(set(R.ranks(s, 0, 1, 3)[0].tolist())) == 3)
    exact, dev = check_unrefined(ctx, cloud, 0.01, hypotheses=1, seed=seed, max_planes=3, min_inliers=3)
    assert dev["n_planes"] == 1 and dev["inliers"].tolist() == [3] and dev["labels"].tolist() == [0, 0, 0] and dev["winners"].tolist() == [0]
    bad = next(s for s in range(100) if len(set(R.ranks(s, 0, 1, 3)[0].tolist())) < 3)          # a repeated draw: nothing is found
    dev = call(ctx, cloud, 0.01, hypotheses=1, seed=bad)
    assert dev["n_planes"] == 0 and dev["labels"].tolist() == [-1, -1, -1]


def test_many_chunks_merged_by_integer_adds(ctx):
    cloud = tilted_planes((40000, 20000), 10000, THR, 70)
    triples, valid, plane4, count = ctx.segment_plane_hypotheses(cloud, THR, 64, 9)
    rt, rv, rp = R.hypotheses(cloud, np.arange(70000), 9, 0, 64)
    assert np.array_equal(triples, rt) and np.array_equal(valid.astype(bool), rv) and (ulps(plane4, rp) <= 1).all()
    assert np.array_equal(count, R.counts(plane4, rv, cloud, THR))
    same = (ulps(plane4, rp) == 0).all(axis=1)
    assert np.array_equal(count[same], R.counts(rp, rv, cloud, THR)[same])
    check_unrefined(ctx, cloud, THR, hypotheses=64, seed=9, max_planes=2, min_inliers=1000)


def test_sixteen_planes_asked_for_on_a_cloud_that_runs_out(ctx):
    rng = np.random.default_rng(4)
    which = rng.permutation(np.repeat([0, 1], [60, 40]))
    cloud = np.concatenate([rng.uniform(-4, 4, (100, 2)), 3.0 * which[:, None]], axis=1).astype(np.float32)
    for refine in (0, 2):
        dev = call(ctx, cloud, 0.01, hypotheses=100, seed=2, refine_iterations=refine, max_planes=16, min_inliers=3)
        assert dev["n_planes"] == 2 and dev["inliers"].tolist() == [60, 40] and np.array_equal(dev["labels"], which) and recount(cloud, dev, 0.01)
    cloud, which = planted_three()
    dev = call(ctx, cloud, 0.01, hypotheses=200, seed=7, refine_iterations=2, max_planes=4, min_inliers=50)
    assert dev["n_planes"] == 3 and dev["inliers"].tolist() == [300, 200, 100] and np.array_equal(dev["labels"], which)


def test_degenerate_clouds(ctx):
    line = np.linspace(0, 1, 50, dtype=np.float32)[:, None] * np.array([[1.0, 2.0, 4.0]], np.float32)
    same = np.tile(np.array([[1.5, -2.25, 3.0]], np.float32), (200, 1))
    for cloud in (line, same):
        dev = call(ctx, cloud, 0.5, hypotheses=64, seed=1, max_planes=3)
        assert dev["n_planes"] == 0 and (dev["labels"] == -1).all() and dev["planes"].shape == (0, 4)
        _, valid, plane4, count = ctx.segment_plane_hypotheses(cloud, 0.5, 64, 1)
        assert not valid.any() and (plane4 == 0).all() and (count == 0).all()


def test_the_axis_rule(ctx):
    cloud, which = axis_case()
    exact, dev = check_unrefined(ctx, cloud, 0.01, hypotheses=300, seed=9, min_inliers=50)
    assert dev["inliers"].tolist() == [300] and np.array_equal(dev["labels"] == 0, which == 1)
    exact, dev = check_unrefined(ctx, cloud, 0.01, hypotheses=300, seed=9, min_inliers=50, axis=[0, 0, 2], min_axis_cosine=0.9)
    assert dev["inliers"].tolist() == [100] and np.array_equal(dev["labels"] == 0, which == 0)
    _, valid, _, _ = ctx.segment_plane_hypotheses(cloud, 0.01, 300, 9, axis=[0, 0, 2], min_axis_cosine=0.9)
    assert np.array_equal(valid.astype(bool), R.hypotheses(cloud, np.arange(400), 9, 0, 300, [0, 0, 2], 0.9)[1])


def raw(ctx, capi, cloud, n=None, thr=THR, hyp=50, seed=1, refine=2, planes=2, min_inliers=3, axis=None, cosine=0.0, null=(), ctx_null=False):
    """mi_segment_plane on sentinel-filled outputs: (rc, message, outputs, all untouched?)"""
    n = len(cloud) if n is None else n
    out = dict(planes4=np.full(4 * 16, -7, np.float32), plane_inliers=np.full(16, -7, np.int32), labels=np.full(max(len(cloud), 1), -7, np.int32),
               rmse=np.full(16, -7, np.float32), winners=np.full(16, -7, np.int32))
    found = C.c_int(-7)
    ptr = {k: (None if k in null else v.ctypes.data) for k, v in out.items()}
    axis = None if axis is None else np.asarray(axis, np.float32)
    rc = capi.segment_plane_raw(None if ctx_null else ctx._h, None if "cloud" in null else cloud.ctypes.data, n, thr, hyp, seed, refine, planes, min_inliers,
                                None if axis is None else axis.ctypes.data, cosine, ptr["planes4"], None if "n_planes" in null else C.addressof(found),
                                ptr["plane_inliers"], ptr["labels"], ptr["rmse"], ptr["winners"])
    untouched = all((v == -7).all() for v in out.values()) and found.value == -7
    return rc, capi.lib().mi_last_error().decode(), dict(out, n_planes=found.value), untouched


def test_the_same_call_twice_gives_the_same_bytes(ctx, capi):
    a, b = raw(ctx, capi, scene(), hyp=H, planes=4, min_inliers=300), raw(ctx, capi, scene(), hyp=H, planes=4, min_inliers=300)
    assert a[0] == b[0] == capi.MI_OK and a[2]["n_planes"] == 3
    for k in a[2]:
        assert np.array_equal(np.asarray(a[2][k]).view(np.uint8) if k != "n_planes" else a[2][k], np.asarray(b[2][k]).view(np.uint8) if k != "n_planes" else b[2][k]), k
    t = ctx.segment_plane_times()
    assert t["total"] > 0 and all(v >= 0 for v in t.values())


def test_dropping_the_optional_outputs_moves_no_bit(ctx, capi):
    full = raw(ctx, capi, scene(), hyp=H, planes=4, min_inliers=300)
    bare = raw(ctx, capi, scene(), hyp=H, planes=4, min_inliers=300, null=("plane_inliers", "labels", "rmse", "winners"))
    assert full[0] == bare[0] == capi.MI_OK and bare[2]["n_planes"] == full[2]["n_planes"] == 3
    assert np.array_equal(full[2]["planes4"].view(np.uint32), bare[2]["planes4"].view(np.uint32))
    assert (full[2]["planes4"][12:] == -7).all() and (full[2]["plane_inliers"][3:] == -7).all() and (full[2]["rmse"][3:] == -7).all() and (full[2]["winners"][3:] == -7).all()
    for k in ("plane_inliers", "labels", "rmse", "winners"):
        assert (bare[2][k] == -7).all()


def test_a_loaded_icp_problem_survives(ctx, capi):
    before, after, _, _ = synth_cloud(3000)
    p = capi.icp_params(max_iterations=6)
    ctx.icp_load(before, after, p)
    ctx.icp_run(6)
    want = ctx.icp_result()
    ctx.icp_load(before, after, p)
    call(ctx, scene(), THR, hypotheses=H, seed=SEED, max_planes=2, min_inliers=300)
    ctx.segment_plane_hypotheses(scene(), THR, 64, 1)
    ctx.icp_run(6)
    got = ctx.icp_result()
    for a, b in zip(got, want):
        assert np.array_equal(np.asarray(a), np.asarray(b))


def test_refusals_leave_the_outputs_untouched(ctx, capi):
    cloud = np.array(scene()[:500])
    nan, big = cloud.copy(), cloud.copy()
    nan[[17, 300], 1] = np.nan
    big[44, 2] = 2e18
    cases = [dict(ctx_null=True), dict(null=("cloud",)), dict(null=("planes4",)), dict(null=("n_planes",)), dict(n=2), dict(thr=0.0), dict(thr=-1.0),
             dict(thr=float("nan")), dict(thr=float("inf")), dict(thr=1e30), dict(hyp=0), dict(hyp=(1 << 22) + 1), dict(refine=-1), dict(refine=9),
             dict(planes=0), dict(planes=17), dict(min_inliers=2), dict(axis=[0, 0, 0], cosine=0.5), dict(axis=[0, np.nan, 1], cosine=0.5),
             dict(axis=[0, 0, 1], cosine=1.0), dict(axis=[0, 0, 1], cosine=-0.1)]
    for kw in cases:
        rc, msg, _, untouched = raw(ctx, capi, cloud, **kw)
        assert rc == capi.MI_ERR_INVALID_ARG and msg.startswith("mi_segment_plane:") and untouched, (kw, rc, msg)
    for bad, index in ((nan, 17), (big, 44)):
        rc, msg, _, untouched = raw(ctx, capi, bad)
        assert rc == capi.MI_ERR_INVALID_ARG and msg.startswith("mi_segment_plane:") and ("point %d " % index) in msg and untouched, msg
    # the cosine is read only with an axis
    assert raw(ctx, capi, cloud, cosine=5.0)[0] == capi.MI_OK
    # the primitive: the same checks, and its window
    triples, valid, plane4, count = np.full(30, -7, np.int32), np.full(10, 7, np.uint8), np.full(40, -7, np.float32), np.full(10, -7, np.int32)
    for n, thr, hyp, first, cnt, data in ((500, THR, 50, -1, 10, cloud), (500, THR, 50, 0, 0, cloud), (500, THR, 50, 45, 10, cloud), (2, THR, 50, 0, 10, cloud),
                                          (500, 0.0, 50, 0, 10, cloud), (500, THR, 0, 0, 10, cloud), (500, THR, 50, 0, 10, nan)):
        rc = capi.segment_plane_hypotheses_raw(ctx._h, data.ctypes.data, n, thr, hyp, 1, None, 0.0, first, cnt, triples.ctypes.data, valid.ctypes.data,
                                               plane4.ctypes.data, count.ctypes.data)
        msg = capi.lib().mi_last_error().decode()
        assert rc == capi.MI_ERR_INVALID_ARG and msg.startswith("mi_segment_plane_hypotheses:"), (n, thr, hyp, first, cnt, msg)
        assert (triples == -7).all() and (valid == 7).all() and (plane4 == -7).all() and (count == -7).all()
