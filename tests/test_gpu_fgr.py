"""GPU suite: mi_fgr_tuples, mi_fgr_system and mi_fgr_register against the numpy restatement of their contract (tests/fgr_reference.py), and
the chain voxel filter -> normals -> FPFH -> mutual match -> mi_fgr_register -> mi_icp_plane_register end to end.  The used list and the
accepted trials are integers and are compared for equality; mu and final_mu bit for bit; every sum against math.fsum of the restatement's
own float64 terms within gamma_k * sum |terms|, k the depth of the library's fixed summation tree (fgr_reference.tree_depth) plus one for
fsum's own rounding, u = 2^-53 -- derived, not tuned; the loop's pose against the restatement's within ten times the restatement's own
spread under a reversed used list.  What the tests measure goes to tests/golden/fgr_measured.json when MISLAM_WRITE_MEASURED is set.
Not covered: the refusal of a distributed context (MI_ERR_STATE) -- no GPU test of this tree shows a cheap way to an exchange context.
The issue's "one lane made non-finite by a huge T" cannot be built: T's entries are finite fp32 and coordinates stay below 1e18, so the
fp64 x stays below 1e58; the huge T is run (every lane finite, the sums of the order of 1e76 and beyond) and the non-finite rule is held on
the restatement alone (tests/test_fgr_abi.py).  Nor can a used list of ONE match: three matches at least are required and a tuple brings
three, so the smallest lists run here hold 3 (both ways).  What a list of one would exercise -- a single row with 63 absent lanes -- the list of 3 does."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

import fgr_reference as F
import plane_reference as P
from conftest import ROOT, synth_cloud
from test_gpu_global_registration import bumpy

pytestmark = pytest.mark.gpu

DELTA = 0.02
MEASURED = {}


def record(key, value):
    MEASURED[key] = max(float(value), MEASURED.get(key, 0.0))
    if os.environ.get("MISLAM_WRITE_MEASURED"):
        with open(os.path.join(ROOT, "tests", "golden", "fgr_measured.json"), "w") as fh:
            json.dump(dict(note="largest figures seen by tests/test_gpu_fgr.py on one MI355X: sums as a share of their derived bound; poses against the restatement", **MEASURED),
                      fh, indent=1, sort_keys=True)


@functools.lru_cache(maxsize=None)
def problem(C_, share, seed, unmatched=0):
    out = F.planted(C_, share, seed, unmatched=unmatched)
    for a in out:
        a.setflags(write=False)
    return out


def pose_gap(R, t, R2, t2):
    return max(np.linalg.norm(np.asarray(R, np.float64) - R2), np.linalg.norm(np.asarray(t, np.float64) - t2))


# ---- the used list
@pytest.mark.parametrize("C_", [3, 63, 64, 65, 1000])
@pytest.mark.parametrize("scale,max_tuples,seed", [(0.95, 1000, 0), (0.5, 7, 0xFEDCBA9876543210), (0.95, 5, 12345)])
def test_tuples_equal_the_restatement(ctx, capi, C_, scale, max_tuples, seed):
    src, tgt, idx, _, _, _ = problem(C_, 0.3, 40 + C_, unmatched=9)
    p = capi.fgr_params(DELTA, tuple_scale=scale, max_tuples=max_tuples, seed=seed)
    used, us, ut, accepted = ctx.fgr_tuples(src, tgt, idx, p)
    ref = F.used_list(src, tgt, idx, scale, max_tuples, 0, seed)
    assert accepted == ref["accepted"] and used == len(ref["used_src"]) == 3 * min(accepted, max_tuples)
    assert np.array_equal(us, ref["used_src"]) and np.array_equal(ut, ref["used_tgt"])
    if C_ >= 63 and max_tuples < 1000:
        assert accepted > max_tuples                                     # this setting truncates


def test_tuples_without_a_filter_are_the_ranks(ctx, capi):
    src, tgt, idx, _, _, _ = problem(65, 0.3, 4, unmatched=5)
    idx = idx.copy()
    idx[[3, 17]] = -1
    used, us, ut, accepted = ctx.fgr_tuples(src, tgt, idx, capi.fgr_params(DELTA, tuple_scale=0.0))
    want = np.flatnonzero(idx >= 0)
    assert used == 63 and accepted == 0 and np.array_equal(us, want) and np.array_equal(ut, idx[want])
    # tuple_trials given: the first trials of the same sequence
    p = capi.fgr_params(DELTA, tuple_trials=500, seed=3)
    used, us, ut, accepted = ctx.fgr_tuples(src, tgt, idx, p)
    ref = F.used_list(src, tgt, idx, 0.95, 1000, 500, 3)
    assert accepted == ref["accepted"] and np.array_equal(us, ref["used_src"]) and np.array_equal(ut, ref["used_tgt"])


def test_no_trial_passes_when_the_clouds_are_scaled_apart(ctx, capi):
    src, tgt, idx, _, _, _ = problem(200, 0.3, 5)
    far = (3 * tgt).astype(np.float32)
    p = capi.fgr_params(DELTA, seed=1)
    used, us, ut, accepted = ctx.fgr_tuples(src, far, idx, p)
    assert used == 0 and accepted == 0 and len(us) == 0
    init = np.eye(4, dtype=np.float32)
    init[:3, 3] = [1, 2, 3]
    for T0 in (None, init):
        R, t, it, err, why, used, mu, w, usrc = ctx.fgr_register(src, far, idx, p, init=T0, want_weights=True)
        assert (it, err, why, used) == (0, 0.0, capi.STOP_NO_PAIRS, 0) and len(w) == 0 and len(usrc) == 0
        assert np.array_equal(R, np.eye(3, dtype=np.float32)) and np.array_equal(t, np.zeros(3) if T0 is None else init[:3, 3])
        assert mu == np.float32(F.scale2(src, far))
    sums, centre, mu = ctx.fgr_system(src, far, idx, p)
    assert not sums.any() and np.array_equal(centre, P.centre(far)) and mu == F.scale2(src, far)


# ---- one linearisation
def synthetic_matches(used, seed):
    """`used` matches with duplicates: source points drawn with repetition are distinct rows, so duplicated MATCHES come from the tuple filter;
    here every third target row is shared by two sources (idx repeats), and a fifth of the matches are wrong"""
    rng = np.random.default_rng(seed)
    src = rng.uniform(-1, 1, (used, 3))
    R0 = F.rotation([0.2, -0.7, 0.4], 0.8)
    tgt = src @ R0.T + np.array([0.3, -0.2, 0.5]) + 0.002 * rng.normal(size=(used, 3))
    idx = np.arange(used, dtype=np.int32)
    idx[rng.permutation(used)[:used // 5]] = rng.integers(0, used, used // 5)
    idx[2::3] = idx[1::3][:len(idx[2::3])]
    return src.astype(np.float32), tgt.astype(np.float32), idx


def check_system(ctx, capi, src, tgt, idx, p, used_ref, T, k, tag):
    sums, centre, mu = ctx.fgr_system(src, tgt, idx, p, T=T, applied_updates=k)
    mu_ref = F.mu_at(F.scale2(src, tgt), p.max_distance, p.division_factor, p.decrease_every, k)
    assert mu == mu_ref                                                  # bit for bit
    T64 = np.eye(4) if T is None else np.asarray(T, np.float32).astype(np.float64)
    ref = F.system(src, tgt, used_ref, T64[:3, :3], T64[:3, 3], mu_ref)
    assert np.array_equal(centre, ref["centre"])
    n_used = len(used_ref["used_src"])
    assert sums[29] == n_used and not sums[30:].any()
    bound = F.gamma(F.tree_depth(n_used) + 1) * ref["abs"]
    gap = np.abs(sums - ref["fsum"])
    worst = float(np.max(np.where(bound > 0, gap / np.where(bound > 0, bound, 1), np.where(gap > 0, np.inf, 0))))
    print("%s: used %d, k %d, mu %.6g, worst |sum - fsum| / bound %.3f, %d of 32 sums bit-equal to the library-order restatement" %
          (tag, n_used, k, mu, worst, int((sums == ref["sums"]).sum())))
    record("system_worst_share_of_bound", worst)
    assert (gap <= bound).all(), (tag, np.flatnonzero(gap > bound), gap, bound)


T_MOVED = np.eye(4, dtype=np.float32)
T_MOVED[:3, :3] = F.rotation([0.5, 0.1, -0.3], 0.6).astype(np.float32)
T_MOVED[:3, 3] = [0.2, -0.1, 0.4]
T_HUGE = np.full((4, 4), 3e38, np.float32) * np.array([[1, -1, 1, 1], [-1, 1, 1, -1], [1, 1, -1, 1], [0, 0, 0, 0]], np.float32)


@pytest.mark.parametrize("used", [3, 63, 64, 65, 200, 70000])
def test_system_equals_the_restatement_per_sum(ctx, capi, used):
    src, tgt, idx = synthetic_matches(used, 70 + used)
    p = capi.fgr_params(DELTA, tuple_scale=0.0)
    ref = F.used_list(src, tgt, idx, 0.0)
    assert len(ref["used_src"]) == used
    for T, k in ((None, 0), (T_MOVED, 0), (T_MOVED, 10000), (T_HUGE, 5)):
        check_system(ctx, capi, src, tgt, idx, p, ref, T, k, "no filter")
    assert F.mu_at(F.scale2(src, tgt), DELTA, 1.4, 4, 10000) <= DELTA * DELTA * 1.0000001       # k = 10 000: mu sits at its floor


def test_system_of_a_single_used_match_and_of_duplicated_matches(ctx, capi):
    # the filter's used list repeats matches: C = 5 true matches, 40 kept trials -> 120 used matches of 5 distinct ones
    src, tgt, idx, _, _, _ = problem(5, 0.0, 8)
    p = capi.fgr_params(DELTA, tuple_scale=0.5, max_tuples=40, seed=2)
    ref = F.used_list(src, tgt, idx, 0.5, 40, 0, 2)
    assert len(ref["used_src"]) == 120 and len(set(ref["used_src"].tolist())) <= 5
    for T, k in ((None, 0), (T_MOVED, 3), (T_MOVED, 10000)):
        check_system(ctx, capi, src, tgt, idx, p, ref, T, k, "duplicates")
    # one kept tuple: three used matches, the smallest list a filter can give; a list of ONE match cannot be asked for (three matches at least)
    p = capi.fgr_params(DELTA, tuple_scale=0.5, max_tuples=1, seed=2)
    check_system(ctx, capi, src, tgt, idx, p, F.used_list(src, tgt, idx, 0.5, 1, 0, 2), T_MOVED, 0, "one tuple")


# ---- the loop
def run(ctx, capi, src, tgt, idx, init=None, **kw):
    p = capi.fgr_params(DELTA, **kw)
    R, t, it, err, why, used, mu, w, usrc = ctx.fgr_register(src, tgt, idx, p, init=init, want_weights=True)
    return dict(R=R, t=t, iterations=it, error=err, stop=why, used=used, final_mu=mu, weights=w, used_src=usrc, T=P.pose44(R, t))


def reference(src, tgt, idx, init=None, reverse=False, **kw):
    used = F.used_list(src, tgt, idx, kw.get("tuple_scale", 0.95), kw.get("max_tuples", 1000), kw.get("tuple_trials", 0), kw.get("seed", 0))
    loop = {k: v for k, v in kw.items() if k in ("division_factor", "decrease_every", "max_iterations", "eps_rotation", "eps_translation")}
    return dict(F.register(src, tgt, used, DELTA, init=init, reverse=reverse, **loop), used_src=used["used_src"])


def against_the_restatement(dev, src, tgt, idx, tag, init=None, **kw):
    ref, rev = reference(src, tgt, idx, init, **kw), reference(src, tgt, idx, init, reverse=True, **kw)
    spread = pose_gap(ref["R"], ref["t"], rev["R"], rev["t"])
    gap = pose_gap(dev["R"], dev["t"], ref["R"].astype(np.float32).astype(np.float64), ref["t"].astype(np.float32).astype(np.float64))
    print("%s: %d iterations, stop %d, |pose - restatement| %.3e, the restatement's own spread %.3e, final mu %.6g" % (tag, dev["iterations"], dev["stop"], gap, spread, dev["final_mu"]))
    record("loop_pose_gap", gap)
    record("loop_restatement_spread", spread)
    assert dev["iterations"] == ref["iterations"] and dev["stop"] == ref["stop"]
    assert dev["final_mu"] == ref["final_mu"] and dev["used"] == len(ref["used_src"]) and np.array_equal(dev["used_src"], ref["used_src"])
    assert gap <= 10 * spread, (gap, spread)
    return ref


@pytest.mark.parametrize("C_,share", [(400, 0.4), (200, 0.6), (65, 0.3)])
@pytest.mark.parametrize("scale", [0.0, 0.95])
def test_planted_problem(ctx, capi, C_, share, scale):
    src, tgt, idx, R0, t0, true = problem(C_, share, 1000 + C_)
    kw = dict(max_iterations=128, tuple_scale=scale, seed=7)
    dev = run(ctx, capi, src, tgt, idx, **kw)
    ref = against_the_restatement(dev, src, tgt, idx, "planted %d / %.0f %% / scale %g" % (C_, 100 * share, scale), **kw)
    assert dev["iterations"] == 128 and dev["stop"] == capi.STOP_MAX_ITERATIONS
    off = pose_gap(dev["R"], dev["t"], R0, t0)
    record("planted_off_truth", off)
    assert off <= 5e-3, off                                             # the issue's condition, independent of the restatement
    assert (dev["weights"][true[dev["used_src"]]] > 0.5).all()            # every true match counts
    assert np.abs(dev["weights"] - ref["weights"]).max() <= 1e-6         # l in [0, 1] as float32, under poses 1e-14 apart
    assert abs(dev["error"] - ref["error"]) <= 1e-6 * max(ref["error"], 1e-30)


def test_loop_settings_and_stops(ctx, capi):
    src, tgt, idx, R0, t0, true = problem(200, 0.3, 77)
    init = np.eye(4, dtype=np.float32)
    init[:3, :3], init[:3, 3] = F.rotation([1, 2, 3], 0.4).astype(np.float32), [0.1, 0.2, -0.3]
    # a start pose; other schedule settings
    kw = dict(max_iterations=40, tuple_scale=0.0, division_factor=2.0, decrease_every=2)
    dev = run(ctx, capi, src, tgt, idx, init=init, **kw)
    against_the_restatement(dev, src, tgt, idx, "init_T", init=init, **kw)
    # max_iterations = 0: init_T comes back
    dev = run(ctx, capi, src, tgt, idx, init=init, max_iterations=0, tuple_scale=0.0)
    assert (dev["iterations"], dev["stop"], dev["error"], dev["used"]) == (0, capi.STOP_MAX_ITERATIONS, 0.0, 200)
    assert np.array_equal(dev["T"], init) and dev["final_mu"] == np.float32(F.scale2(src, tgt))
    ref = reference(src, tgt, idx, init=init, max_iterations=0, tuple_scale=0.0)
    assert np.abs(dev["weights"] - ref["weights"]).max() <= 1e-6
    # eps > 0 stops where the restatement stops -- before the schedule is through
    kw = dict(max_iterations=128, tuple_scale=0.0, eps_rotation=1e-3, eps_translation=1e-3)
    dev = run(ctx, capi, src, tgt, idx, **kw)
    ref = against_the_restatement(dev, src, tgt, idx, "eps", **kw)
    assert dev["stop"] == capi.STOP_CONVERGED and 0 < dev["iterations"] < 128


def test_collinear_matches_are_degenerate(ctx, capi):
    s = np.linspace(-1, 1, 40)[:, None] * np.array([[1.0, 2.0, -0.5]]) + np.array([[0.25, 0.5, 0.75]])
    src, tgt, idx = s.astype(np.float32), (s + 0.125).astype(np.float32), np.arange(40, dtype=np.int32)
    kw = dict(max_iterations=20, tuple_scale=0.0)
    dev = run(ctx, capi, src, tgt, idx, **kw)
    ref = reference(src, tgt, idx, **kw)
    assert dev["stop"] == ref["stop"] == capi.STOP_DEGENERATE and dev["iterations"] == ref["iterations"]
    assert np.array_equal(dev["T"], P.pose44(ref["R"], ref["t"])) or pose_gap(dev["R"], dev["t"], ref["R"], ref["t"]) <= 1e-6
    if dev["iterations"] == 0:
        assert np.array_equal(dev["T"], np.eye(4, dtype=np.float32))     # the pose before that iteration
    assert dev["final_mu"] == ref["final_mu"]


def test_same_bits_whatever_the_batching_and_on_every_call(ctx, capi):
    src, tgt, idx, _, _, _ = problem(400, 0.4, 1400)
    outs = [run(ctx, capi, src, tgt, idx, max_iterations=37, seed=5, sync_every=s) for s in (1, 4, 64, 0, 4)]
    for o in outs[1:]:
        for k in ("R", "t", "weights", "used_src"):
            assert np.array_equal(np.asarray(o[k]).view(np.uint8), np.asarray(outs[0][k]).view(np.uint8)), k
        assert (o["iterations"], o["stop"], o["used"]) == (outs[0]["iterations"], outs[0]["stop"], outs[0]["used"])
        assert np.float32(o["error"]).tobytes() == np.float32(outs[0]["error"]).tobytes() and o["final_mu"].tobytes() == outs[0]["final_mu"].tobytes()
    times = ctx.fgr_register_times()
    assert set(times) == {"workspace", "upload", "check", "tuples", "gather", "iterations", "download", "total"} and times["total"] > 0


def test_a_loaded_icp_problem_survives(ctx, capi):
    before, after, _, _ = synth_cloud(3000)
    params = capi.icp_params(max_iterations=6)
    ctx.icp_load(before, after, params)
    ctx.icp_run(6)
    want = ctx.icp_result()
    ctx.icp_load(before, after, params)
    src, tgt, idx, _, _, _ = problem(200, 0.3, 77)
    run(ctx, capi, src, tgt, idx, max_iterations=8)
    ctx.fgr_tuples(src, tgt, idx, capi.fgr_params(DELTA))
    ctx.fgr_system(src, tgt, idx, capi.fgr_params(DELTA))
    ctx.icp_run(6)
    got = ctx.icp_result()
    for a, b in zip(got, want):
        assert np.array_equal(np.asarray(a), np.asarray(b))


# ---- refusals that need a context: nothing is written, the message names the entry point
def _bad_cases():
    yield "n", dict(n=0), "empty cloud"
    yield "max_distance", dict(max_distance=0.0), "max_distance"
    yield "max_distance_nan", dict(max_distance=float("nan")), "max_distance"
    yield "division_factor", dict(division_factor=1.0), "division_factor"
    yield "decrease_every", dict(decrease_every=0), "decrease_every"
    yield "max_iterations", dict(max_iterations=-1), "max_iterations"
    yield "tuple_scale", dict(tuple_scale=1.0), "tuple_scale"
    yield "max_tuples", dict(max_tuples=0), "max_tuples"
    yield "max_tuples_high", dict(max_tuples=(1 << 20) + 1), "max_tuples"
    yield "tuple_trials", dict(tuple_trials=(1 << 22) + 1), "tuple_trials"
    yield "eps", dict(eps_rotation=-1.0), "eps_rotation"
    yield "sync_every", dict(sync_every=-1), "sync_every"
    yield "idx_high", dict(idx={5: 10 ** 6, 9: -2}), "idx[5]"
    yield "idx_low", dict(idx={9: -2}), "idx[9]"
    yield "few", dict(idx={i: -1 for i in range(2, 30)}), "fewer than 3"
    yield "init_T", dict(T=4), "transform entry 4"
    yield "src_nan", dict(src=(7, float("nan"))), "src_xyz point 7"
    yield "tgt_big", dict(tgt=(3, 2e18)), "tgt_xyz point 3"


@pytest.mark.parametrize("name,change,needle", list(_bad_cases()), ids=[c[0] for c in _bad_cases()])
def test_invalid_arguments_write_nothing(ctx, capi, name, change, needle):
    rng = np.random.default_rng(1)
    src, tgt, idx = rng.uniform(0, 1, (30, 3)).astype(np.float32), rng.uniform(0, 1, (30, 3)).astype(np.float32), np.arange(30, dtype=np.int32)
    fields = {k: v for k, v in change.items() if k not in ("n", "idx", "T", "src", "tgt", "max_distance")}
    p = capi.fgr_params(change.get("max_distance", DELTA), **fields)
    for i, j in change.get("idx", {}).items():
        idx[i] = j
    if "src" in change:
        src[change["src"][0], 1] = change["src"][1]
    if "tgt" in change:
        tgt[change["tgt"][0], 2] = change["tgt"][1]
    T0 = np.eye(4, dtype=np.float32).T.reshape(16).copy()
    if "T" in change:
        T0[change["T"]] = np.inf
    n = change.get("n", 30)
    T, w, us, ut = np.full(16, -7, np.float32), np.full(3000, -7, np.float32), np.full(3000, -7, np.int32), np.full(3000, -7, np.int32)
    it, why, used, acc, err, mu = C.c_int(-7), C.c_int(-7), C.c_int(-7), C.c_int(-7), C.c_float(-7), C.c_float(-7)
    sums, centre, mu64 = np.full(32, -7.0), np.full(3, -7, np.float32), C.c_double(-7)
    h = ctx._h
    calls = [("mi_fgr_register", lambda: capi.fgr_register_raw(h, src.ctypes.data, n, tgt.ctypes.data, 30, idx.ctypes.data, C.addressof(p), T0.ctypes.data, T.ctypes.data,
                                                               C.addressof(it), C.addressof(err), C.addressof(why), C.addressof(used), C.addressof(mu), w.ctypes.data, us.ctypes.data)),
             ("mi_fgr_system", lambda: capi.fgr_system_raw(h, src.ctypes.data, n, tgt.ctypes.data, 30, idx.ctypes.data, C.addressof(p), T0.ctypes.data, 0, sums.ctypes.data,
                                                           centre.ctypes.data, C.addressof(mu64)))]
    if "T" not in change:
        calls.append(("mi_fgr_tuples", lambda: capi.fgr_tuples_raw(h, src.ctypes.data, n, tgt.ctypes.data, 30, idx.ctypes.data, C.addressof(p), C.addressof(used), us.ctypes.data,
                                                                   ut.ctypes.data, C.addressof(acc))))
    for who, call in calls:
        rc = call()
        msg = capi.lib().mi_last_error().decode()
        assert rc == capi.MI_ERR_INVALID_ARG and msg.startswith(who + ":") and needle in msg, (who, rc, msg)
    assert (T == -7).all() and (w == -7).all() and (us == -7).all() and (ut == -7).all() and (sums == -7).all() and (centre == -7).all()
    assert [it.value, why.value, used.value, acc.value, err.value, mu.value, mu64.value] == [-7] * 7


def test_null_outputs_and_negative_updates_are_refused(ctx, capi):
    src, tgt, idx, _, _, _ = problem(65, 0.3, 1065)
    p = capi.fgr_params(DELTA)
    used, sums = C.c_int(-7), np.full(32, -7.0)
    rc = capi.fgr_register_raw(ctx._h, src.ctypes.data, 65, tgt.ctypes.data, 65, idx.ctypes.data, C.addressof(p), None, None, None, None, None, C.addressof(used), None, None, None)
    assert rc == capi.MI_ERR_INVALID_ARG and capi.lib().mi_last_error().decode().startswith("mi_fgr_register: null out_T or used") and used.value == -7
    rc = capi.fgr_system_raw(ctx._h, src.ctypes.data, 65, tgt.ctypes.data, 65, idx.ctypes.data, C.addressof(p), None, -1, sums.ctypes.data, None, None)
    assert rc == capi.MI_ERR_INVALID_ARG and "applied_updates" in capi.lib().mi_last_error().decode() and (sums == -7).all()
    # the optional outputs may all be NULL
    T = np.zeros(16, np.float32)
    rc = capi.fgr_register_raw(ctx._h, src.ctypes.data, 65, tgt.ctypes.data, 65, idx.ctypes.data, C.addressof(p), None, T.ctypes.data, None, None, None, C.addressof(used), None, None, None)
    assert rc == capi.MI_OK and used.value > 0 and T[15] == 1


# ---- the chain
def test_chain_from_raw_scans_to_a_refined_pose(ctx, capi):
    """voxel filter -> normals -> FPFH -> mutual match -> mi_fgr_register -> mi_icp_plane_register from its out_T.  No test runs the same chain
    through mi_ransac_register (tests/test_gpu_global_registration.py stops at the start pose and brings analytic normals), so the bound is the
    issue's other one: ten times what the plane registration itself reaches from the TRUE start on the same clouds."""
    p, _ = bumpy(9000)
    R0, t0 = F.rotation([0.3, -0.5, 0.8], 1.0), np.array([0.3, -0.2, 0.5])
    rng = np.random.default_rng(5)
    raw_src = (p + 0.0005 * rng.normal(size=p.shape)).astype(np.float32)
    raw_tgt = ((p @ R0.T + t0)[rng.permutation(len(p))] + 0.0005 * rng.normal(size=p.shape)).astype(np.float32)
    src, tgt = ctx.voxel_downsample(raw_src, 0.07), ctx.voxel_downsample(raw_tgt, 0.07)
    assert 1200 <= len(src) <= 4000 and 1200 <= len(tgt) <= 4000, (len(src), len(tgt))
    src_n = ctx.estimate_normals(src, 12, viewpoint=src.mean(axis=0))
    tgt_n = ctx.estimate_normals(tgt, 12, viewpoint=tgt.mean(axis=0))
    idx = ctx.feature_match(ctx.fpfh_features(src, src_n, 24), ctx.fpfh_features(tgt, tgt_n, 24), mutual=True)
    image = src.astype(np.float64) @ R0.T + t0
    close = (idx >= 0) & (np.linalg.norm(image - tgt[np.maximum(idx, 0)], axis=1) <= 0.07)
    fgr = capi.fgr_params(0.035, seed=1)
    R, t, it, err, why, used, mu = ctx.fgr_register(src, tgt, idx, fgr)
    start = pose_gap(R, t, R0, t0)
    plane = capi.plane_params(max_distance_squared=0.14 ** 2)
    T_true = np.eye(4, dtype=np.float32)
    T_true[:3, :3], T_true[:3, 3] = R0, t0
    Rt, tt, itt, errt, whyt = ctx.icp_plane_register(src, tgt, tgt_n, plane, init=T_true)
    Rf, tf, itf, errf, whyf = ctx.icp_plane_register(src, tgt, tgt_n, plane, init=P.pose44(R, t))
    own, final = pose_gap(Rt, tt, R0, t0), pose_gap(Rf, tf, R0, t0)
    print("chain: %d / %d points, %d matches of which %d within a voxel of their image; FGR used %d, %d iterations, stop %d, off truth %.3e; "
          "plane ICP from the true start %.3e off truth (%d iterations), from FGR's pose %.3e (%d iterations)" %
          (len(src), len(tgt), (idx >= 0).sum(), close.sum(), used, it, why, start, own, itt, final, itf))
    record("chain_fgr_off_truth", start)
    record("chain_plane_from_truth_off_truth", own)
    record("chain_final_off_truth", final)
    assert whyf in (capi.STOP_CONVERGED, capi.STOP_MAX_ITERATIONS)
    assert final <= 10 * own, (final, own)
