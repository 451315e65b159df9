"""GPU suite of mi_pose_graph_optimize and mi_pose_graph_system off their happy and small paths, on the cases of
tests/pose_graph_scale_cases.py (held to their names, margins and plan values on the CPU by tests/test_pose_graph_scale_cases.py).

The bounds (none of them taken from what the device gives):
  the loop     stop reason, linearisations, accepted steps, inner iterations and the final lambda exactly the restatement's: its own decisions
               are no near ties (every trial 1e-6 or more from one, the same trajectory in a second edge order).  Final cost and poses within
               100 x the restatement's own spread between its two edge orders (LOOP_SPREAD), over floors of 1e-12 relative and absolute: the
               device's order of a sum is a third one.  w and chi2 against the restatement's edge terms AT THE POSES THAT CAME BACK, within
               BAR = 1e-12 max(1, max |ref|): an array of another linearisation or of a rejected candidate is off by 1e-3 and more.
  the solve    iterations exactly; x within 100 x the two-order spread of x (SOLVE_SPREAD), floor 1e-12, of max |x|
  shapes       tests/test_gpu_pose_graph.py's: every output and H p within BAR, the cost within BAR E, the solve's true residual within
               10 x its tolerance; isolated nodes exactly 0; same input, same bytes
Measured on an MI355X when the suite was written: DESIGN.md, "K56 - K63 pose-graph optimisation"."""
import ctypes as C

import numpy as np
import pytest

import pose_graph_reference as P
import pose_graph_scale_cases as S
from test_gpu_pose_graph import BAR, optimise, outputs_bytes, ratio, run_system, tri
from test_pose_graph_scale_cases import LOOP_SPREAD, SOLVE_SPREAD, bits

pytestmark = pytest.mark.gpu

MARGIN, FLOOR = 100.0, 1e-12


# ---- A. the loop, branch by branch
@pytest.mark.parametrize("name", list(S.LOOP))
def test_loop_branches(ctx, capi, name):
    g, ref = S.loop_graph(), S.loop_run(name)
    R0, t0 = S.loop_start(name)
    R, t, w, chi2, rep = optimise(ctx, capi, dict(g, R0=R0, t0=t0), **S.loop_params(name))
    F0, F, linearisations, accepted, inner, lam, stop, rel = ref["report"]
    here = P.edge_terms(R, t, g["src"], g["tgt"], g["Rz"], g["tz"], g["info"], g["uncertain"], g["mu"])
    cost = abs(rep["final_cost"] - F) / F
    pose = float(max(np.abs(R - ref["R"]).max(), np.abs(t - ref["t"]).max()))
    dw, dchi2 = ratio(w, here["w"]), ratio(chi2, here["chi2"])
    print("%s: %s; against the restatement: cost %.3g, poses %.3g, pcg_residual %.3g against %.3g; w %.3g and chi2 %.3g at the returned poses"
          % (name, rep, cost, pose, rep["pcg_residual"], rel, dw, dchi2))
    assert (rep["stop_reason"], rep["linearisations"], rep["accepted"], rep["pcg_iterations"]) == (stop, linearisations, accepted, inner)
    assert bits(rep["lambda"]) == bits(lam)
    assert abs(rep["initial_cost"] - F0) <= BAR * F0 * len(g["src"])
    assert cost <= max(MARGIN * LOOP_SPREAD[name][0], FLOOR) and pose <= max(MARGIN * LOOP_SPREAD[name][1], FLOOR)
    assert dw <= BAR and dchi2 <= BAR
    # the last solve's |r| / |g|: 100 x the restatement's own difference between its two orders, or the 1e-6 to which the case's decisions were
    # held on the CPU -- the figure of any other solve of the run differs in its first digits
    assert abs(rep["pcg_residual"] - rel) <= max(MARGIN * abs(S.loop_run(name, True)["report"][7] - rel), 1e-6 * rel)
    if accepted == 0:                                          # nothing taken: the poses as given, bit for bit, and the start's cost
        assert np.array_equal(bits(R), bits(R0)) and np.array_equal(bits(t), bits(t0)) and rep["final_cost"] == rep["initial_cost"]
    if name == "no_inner_iterations":
        assert rep["pcg_residual"] == 1.0


def test_out_poses_may_alias_poses(ctx, capi):
    name = "max_iterations_3"
    g = S.loop_graph()
    R0, t0 = S.loop_start(name)
    plain = optimise(ctx, capi, dict(g, R0=R0, t0=t0), **S.loop_params(name))
    params = capi.pose_graph_params(**S.loop_params(name))
    poses, Z, info = P.to16(R0, t0).copy(), P.to16(g["Rz"], g["tz"]), np.ascontiguousarray(g["info"]).reshape(-1, 36)
    src, tgt, unc = np.ascontiguousarray(g["src"], np.int32), np.ascontiguousarray(g["tgt"], np.int32), np.ascontiguousarray(g["uncertain"], np.uint8)
    E = len(src)
    w, chi2, report = np.empty(E), np.empty(E), np.zeros(8)
    rc = capi.pose_graph_optimize_raw(ctx._h, poses.ctypes.data, len(poses), src.ctypes.data, tgt.ctypes.data, Z.ctypes.data, info.ctypes.data, unc.ctypes.data, E,
                                      C.addressof(params), poses.ctypes.data, w.ctypes.data, chi2.ctypes.data, report.ctypes.data)
    assert rc == capi.MI_OK, capi.lib().mi_last_error().decode()
    R, t = P.from16(poses)
    assert np.array_equal(bits(R), bits(plain[0])) and np.array_equal(bits(t), bits(plain[1])) and plain[4]["accepted"] == 3
    assert np.array_equal(bits(w), bits(plain[2])) and np.array_equal(bits(chi2), bits(plain[3])) and report[1] == plain[4]["final_cost"]
    assert np.array_equal(poses[:, [3, 7, 11, 15]], np.tile([0.0, 0.0, 0.0, 1.0], (len(poses), 1)))


# ---- B. the inner solve's chunking and stop
def solve(ctx, capi, name, tol, cap, lam=S.SOLVE_LAMBDA):
    return run_system(ctx, capi, S.system_graph(name), solve=True, lambda0=lam, tol=tol, cap=cap, p=False)


def x_bound(name, kind, key):
    return max(MARGIN * SOLVE_SPREAD[(name, kind, key)], FLOOR)


def residual_bound(trace, permuted_trace):
    """for the solve's last |r| / |g|: 100 x the restatement's own difference between its two edge orders, floor 1e-12 relative"""
    return max(MARGIN * abs(trace[-1] - permuted_trace[-1]), FLOOR * trace[-1])


@pytest.mark.parametrize("name", ["ring60", "random300"])
def test_solves_end_at_their_cap(ctx, capi, name):
    for cap in S.SOLVE_CAPS:
        x, it, trace = S.solve_run(name, 0.0, cap)
        o = solve(ctx, capi, name, 0.0, cap)
        off = float(np.abs(o["x"] - x).max() / np.abs(x).max())
        print("%s, cap %d: %d iterations, |r| / |g| %.6e against %.6e, x off by %.3g of max |x|" % (name, cap, o["pcg_iterations"], o["pcg_residual"], trace[-1], off))
        assert o["pcg_iterations"] == cap == it
        assert off <= x_bound(name, "cap", cap)
        assert abs(o["pcg_residual"] - trace[-1]) <= residual_bound(trace, S.solve_run(name, 0.0, cap, True)[2])


@pytest.mark.parametrize("name", ["ring60", "random300"])
def test_solves_end_inside_a_chunk(ctx, capi, name):
    """The tolerance is met inside the first chunk of 16 (lambda 0.1) and inside the second (lambda 1e-3); the iterations enqueued behind the
    stop must leave x and the count alone."""
    tol, cap = S.LOOSE
    for lam in S.LOOSE_LAMBDAS:
        x, it, trace = S.solve_run(name, tol, cap, False, lam)
        o = solve(ctx, capi, name, tol, cap, lam)
        off = float(np.abs(o["x"] - x).max() / np.abs(x).max())
        print("%s, lambda %g: %d iterations against %d, |r| / |g| %.6e against %.6e, x off by %.3g of max |x|" % (name, lam, o["pcg_iterations"], it, o["pcg_residual"], trace[-1], off))
        assert o["pcg_iterations"] == it
        assert off <= x_bound(name, "loose", lam)
        assert abs(o["pcg_residual"] - trace[-1]) <= residual_bound(trace, S.solve_run(name, tol, cap, True, lam)[2])


@pytest.mark.parametrize("name", ["ring60", "random300"])
def test_a_tolerance_of_one_stops_at_begin(ctx, capi, name):
    for tol in (1.0, 3.0):
        o = solve(ctx, capi, name, tol, 200)
        assert o["pcg_iterations"] == 0 and not o["x"].any() and o["pcg_residual"] == 1.0
    o = solve(ctx, capi, name, 0.0, 0)                        # and a cap of 0
    assert o["pcg_iterations"] == 0 and not o["x"].any() and o["pcg_residual"] == 1.0


# ---- C. shapes
def check_system(g, o, lam, tag):
    """every output of one linearisation against the restatement, as test_system_per_element holds them; with g["nodes"] the used nodes
    against the compacted restatement and every other node exactly 0"""
    t, nodes = g["terms"], g["nodes"]
    rows = slice(None) if nodes is None else nodes
    Hp = S.product(g, lam, g["p"])
    want = dict(r=(o["r"], t["r"]), chi2=(o["chi2"], t["chi2"]), w=(o["w"], t["w"]), M=(o["M"], tri(t["M"])), h=(o["h"], t["h"]),
                diag=(o["diag"][rows], tri(g["D"])), g=(o["g"][rows], g["g"]), Hp=(o["Hp"][rows], Hp[rows]))
    worst = {k: ratio(dev, ref) for k, (dev, ref) in want.items()}
    print("%s: worst |dev - ref| / max(1, max |ref|): %s" % (tag, ", ".join("%s %.2e" % kv for kv in worst.items())))
    assert abs(o["cost"] - t["cost"]) <= BAR * max(1.0, t["cost"]) * len(g["src"])     # (a sum of E shares)
    assert (o["Hp"][g["ref"]] == 0.0).all()
    for k, v in worst.items():
        assert v <= BAR, (k, v)
    if nodes is not None:
        isolated = np.ones(len(g["R"]), bool)
        isolated[nodes] = False
        for k in ("diag", "g", "Hp"):
            assert not o[k][isolated].any(), k
    return worst


@pytest.mark.parametrize("V", S.SORT_BITS_V)
def test_every_width_of_the_incidence_sort(ctx, capi, V):
    g = S.system_graph(("sort_bits", V))
    lam = 1e-3
    last = V == S.SORT_BITS_V[-1]
    o = run_system(ctx, capi, g, solve=last, lambda0=lam, tol=0.0, cap=20)
    check_system(g, o, lam, "V = %d (%d bits)" % (V, S.sort_bits(V)))
    if last:                                                   # 20 iterations at tolerance 0: one chunk and a quarter
        nodes = g["nodes"]
        (x, it), (x2, _) = S.compact_solve(("sort_bits", V), lam, 20), S.compact_solve(("sort_bits", V), lam, 20, True)
        spread = float(np.abs(x - x2).max() / np.abs(x).max())
        isolated = np.ones(V, bool)
        isolated[nodes] = False
        off = float(np.abs(o["x"][nodes] - x).max() / np.abs(x).max())
        print("V = %d: %d iterations, x off by %.3g of max |x|, the restatement's two orders by %.3g" % (V, o["pcg_iterations"], off, spread))
        assert o["pcg_iterations"] == it == 20 and not o["x"][isolated].any()
        assert off <= max(MARGIN * spread, FLOOR)
        again = run_system(ctx, capi, g, solve=True, lambda0=lam, tol=0.0, cap=20)
        assert outputs_bytes(o) == outputs_bytes(again) and o["cost"] == again["cost"]


def test_the_wide_system(ctx, capi):
    g = S.system_graph("wide")
    lam = 1e-3
    o = run_system(ctx, capi, g, solve=True, lambda0=lam)
    check_system(g, o, lam, "wide")
    x = o["x"]
    assert (x[g["ref"]] == 0.0).all()
    rhs = -g["g"].copy()
    rhs[g["ref"]] = 0.0
    rel = float(np.linalg.norm(S.product(g, lam, x) - rhs) / np.linalg.norm(rhs))
    print("wide: %d inner iterations, true |A x + g| / |g| = %.3e, the recurrence's %.3e" % (o["pcg_iterations"], rel, o["pcg_residual"]))
    assert rel <= 10 * 1e-10, rel
    again = run_system(ctx, capi, g, solve=True, lambda0=lam)
    assert outputs_bytes(o) == outputs_bytes(again) and o["cost"] == again["cost"] and o["pcg_iterations"] == again["pcg_iterations"]


def test_the_wide_graph_converges(ctx, capi):
    """The bound on the poses is test_consistent_graphs_converge's, 1e-8; the cost at which the run may stop is derived from it, because
    1e-18 F_initial does not imply it on a map this wide: the softest error is a rigid turn of the whole map about the reference node by an
    angle a, which moves a pose entry by a L (L: the farthest node's distance from the reference, 11.3 here) and is paid for by the
    reference's own edges alone, a^2 times the smallest eigenvalue of their information (6 and more: tests/pose_graph_reference.py,
    random_information) each.  So F <= 6 degree(ref) (1e-8 / L)^2 is what an error below 1e-8 needs -- 1.4e-17, 1.8e-23 F_initial; at 1e-18 F_initial
    the device stopped at F = 1.9e-16 with the worst entry 1.8e-8 off.  The floor of F by the residuals' roundoff, E 6 10 (1e-15)^2 = 8e-24,
    lies six decades below that."""
    g = S.wide_consistent()
    F0 = P.edge_terms(g["R0"], g["t0"], g["src"], g["tgt"], g["Rz"], g["tz"], g["info"])["cost"]
    ref = g["ref"]
    L = float(np.linalg.norm(g["t"] - g["t"][ref], axis=1).max())
    degree = int((g["src"] == ref).sum() + (g["tgt"] == ref).sum())
    enough = 6.0 * degree * (1e-8 / L) ** 2
    print("wide: L = %.3g, degree(ref) = %d, absolute_cost %.3g = %.3g F_initial" % (L, degree, enough, enough / F0))
    R, t, w, chi2, rep = optimise(ctx, capi, g, absolute_cost=enough, max_pcg_iterations=2000, reference_node=ref)
    err = max(np.abs(R - g["R"]).max(), np.abs(t - g["t"]).max())
    print("wide at 0.05: %s, worst pose entry %.3g" % (rep, err))
    assert abs(rep["initial_cost"] - F0) <= 1e-12 * F0 * len(g["src"])
    assert rep["stop_reason"] == capi.STOP_CONVERGED and rep["linearisations"] <= 12 and err <= 1e-8
    assert (w == 1.0).all() and np.isfinite(chi2).all()


def test_an_edge_without_residual(ctx, capi):
    g = S.system_graph("zero_edge")
    o = run_system(ctx, capi, g, lambda0=1e-3)
    check_system(g, o, 1e-3, "zero edge")
    assert not o["r"][0].any() and o["chi2"][0] == 0.0 and o["w"][0] == 1.0
    assert np.isfinite(o["M"][0]).all() and np.isfinite(o["h"][0]).all() and np.abs(o["M"][0]).max() > 0


def test_alternating_calls_keep_no_buffers(ctx, capi):
    wide, sparse = S.system_graph("wide"), S.system_graph(("sort_bits", S.SORT_BITS_V[-1]))
    run_system(ctx, capi, wide, p=False)
    run_system(ctx, capi, sparse, p=False)
    before = capi.selftest_live_buffers()
    for k in range(10):
        run_system(ctx, capi, wide if k % 2 == 0 else sparse, p=False)
    assert capi.selftest_live_buffers() <= before
