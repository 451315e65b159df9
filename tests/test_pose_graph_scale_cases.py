"""CPU suite: every case of tests/pose_graph_scale_cases.py is what it is named for, shown with tests/pose_graph_reference.py alone.

The loop cases: an exact comparison of a device's decisions with the restatement's is only valid where the restatement's own decisions are
no near ties, so for every case (1) every trial step has |F_new - F| / F >= 1e-6 -- or, where the inner solve made no iteration, F_new is F
bit for bit: x = 0 leaves every pose's bits, so the candidate's cost is the same arithmetic on the same numbers, on the device as here, and
`F_new < F` is false without any rounding in play; (2) the trajectory (each trial's outcome, lambda and inner iterations, the report's
integers and lambda) is the same with the edges in a second, permuted order; (3) the trace shows what the case is named for.

LOOP_SPREAD and SOLVE_SPREAD are what these tests measured between the restatement's two edge orders when they were written (numpy 64-bit):
the roundoff scale of a final cost, of final poses and of an inner solve's x.  The GPU suite's bounds are 100 x them, over floors of 1e-12
(tests/test_gpu_pose_graph_scale.py); here a run may differ from its record by an order of magnitude, as on another BLAS."""
import numpy as np
import pytest

import pose_graph_reference as P
import pose_graph_scale_cases as S

TIE = 1e-6
# name -> (relative difference of the final costs, worst difference of a pose entry)
LOOP_SPREAD = {
    "rejected_then_accepted": (6.73e-10, 1.05e-09),          # 19 trial steps of 40 inner iterations each: every inexact step carries the last one's bits on
    "error_increased_at_once": (0.0, 0.0),
    "error_increased_after_accepting": (2.40e-13, 4.48e-11),
    "max_iterations_1": (1.09e-14, 7.37e-14),
    "max_iterations_3": (6.45e-14, 1.57e-12),
    "max_iterations_0": (0.0, 0.0),
    "no_inner_iterations": (0.0, 0.0),
}
# (graph, "cap", cap) at tolerance 0 and (graph, "loose", lambda) at S.LOOSE -> max |x - x'| / max |x|
SOLVE_SPREAD = {
    ("ring60", "cap", 1): 1.06e-15, ("ring60", "cap", 15): 1.51e-15, ("ring60", "cap", 16): 1.61e-15, ("ring60", "cap", 17): 1.63e-15,
    ("ring60", "cap", 33): 2.44e-15, ("ring60", "loose", 0.1): 7.05e-16, ("ring60", "loose", 1e-3): 2.25e-15,
    ("random300", "cap", 1): 8.55e-16, ("random300", "cap", 15): 2.73e-15, ("random300", "cap", 16): 2.77e-15, ("random300", "cap", 17): 2.73e-15,
    ("random300", "cap", 33): 2.57e-15, ("random300", "loose", 0.1): 1.23e-15, ("random300", "loose", 1e-3): 2.64e-15,
}
SOLVE_GRAPHS = ("ring60", "random300")


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def pattern(run):
    return "".join("A" if r["accepted"] else "r" for r in run["trace"])


def within_a_decade(measured, recorded):
    return measured <= 10.0 * recorded + 1e-15


@pytest.mark.parametrize("name", list(S.LOOP))
def test_loop_case_margins_and_names(name):
    g, a, b = S.loop_graph(), S.loop_run(name), S.loop_run(name, True)
    F0, F, linearisations, accepted, inner, lam, stop, rel = a["report"]
    pat = pattern(a)
    cost, pose = S.loop_spread(name)
    print("%-32s %s stop %d, %d linearisations, %d accepted, %d inner, lambda %.17g, cost %.9g -> %.9g; two orders: cost %.3g, poses %.3g"
          % (name, pat or "-", stop, linearisations, accepted, inner, lam, F0, F, cost, pose))
    # (1) no near tie
    for r in a["trace"] + b["trace"]:
        if r["inner"] == 0:
            assert bits(r["F_new"]) == bits(r["F"])
        else:
            assert abs(r["F_new"] - r["F"]) / r["F"] >= TIE, r
    # (2) the same trajectory in another summation order
    assert S.decisions(a) == S.decisions(b)
    assert within_a_decade(cost, LOOP_SPREAD[name][0]) and within_a_decade(pose, LOOP_SPREAD[name][1])
    # (3) the name
    R0, t0 = S.loop_start(name)
    kw = S.loop_params(name)
    lambda0 = kw.get("lambda0", P.DEFAULTS["lambda0"])
    at_start = P.edge_terms(R0, t0, g["src"], g["tgt"], g["Rz"], g["tz"], g["info"], g["uncertain"], g["mu"])
    assert linearisations == 1 + sum(r["accepted"] for r in a["trace"][:-1])                   # (the step that stops the run is not linearised again)
    assert accepted == pat.count("A") and inner == sum(r["inner"] for r in a["trace"])
    if name == "rejected_then_accepted":
        assert "rrA" in pat and pat.index("rrA") > 0 and stop == P.STOP_CONVERGED          # accepted steps on both sides of the rejected ones
        assert lam == S.LAMBDA_MIN and a["trace"][-1]["lam"] / 10.0 < S.LAMBDA_MIN             # the floor held the last division back
        assert F <= kw["absolute_cost"] < a["trace"][-1]["F"] and not (F <= kw["absolute_cost"] * (1 + TIE) and F >= kw["absolute_cost"] * (1 - TIE))
        assert kw["max_pcg_iterations"] % S.SYNC_EVERY != 0 and all(r["inner"] == kw["max_pcg_iterations"] for r in a["trace"])
    elif name == "error_increased_at_once":
        assert pat == "r" * S.MAX_REJECTIONS and stop == P.STOP_ERROR_INCREASED and linearisations == 1 and accepted == 0
        want = lambda0
        for _ in range(S.MAX_REJECTIONS - 1):
            want *= 10.0
        assert lam == want and bits(a["R"]).tolist() == bits(R0).tolist() and bits(a["w"]).tolist() == bits(at_start["w"]).tolist()
    elif name == "error_increased_after_accepting":
        assert pat.endswith("A" + "r" * S.MAX_REJECTIONS) and len(pat) > S.MAX_REJECTIONS + 1 and stop == P.STOP_ERROR_INCREASED
        assert linearisations == accepted + 1                                                   # the last accepted step was linearised again
        assert kw["max_pcg_iterations"] % S.SYNC_EVERY != 0
    elif name in ("max_iterations_1", "max_iterations_3"):
        assert stop == P.STOP_MAX_ITERATIONS and pat.endswith("A") and linearisations == kw["max_iterations"] == accepted
        assert ("r" in pat) == (name == "max_iterations_3")
    elif name == "max_iterations_0":
        assert pat == "" and stop == P.STOP_MAX_ITERATIONS and linearisations == 1 and accepted == 0 and inner == 0 and lam == lambda0 and F == F0
        assert bits(a["R"]).tolist() == bits(R0).tolist() and bits(a["t"]).tolist() == bits(t0).tolist()
        assert bits(a["w"]).tolist() == bits(at_start["w"]).tolist() and bits(a["chi2"]).tolist() == bits(at_start["chi2"]).tolist()
    elif name == "no_inner_iterations":
        assert pat == "r" * S.MAX_REJECTIONS and stop == P.STOP_ERROR_INCREASED and inner == 0 and rel == 1.0 and F == F0
        want = lambda0
        for _ in range(S.MAX_REJECTIONS - 1):
            want *= 10.0
        assert lam == want and bits(a["R"]).tolist() == bits(R0).tolist() and bits(a["t"]).tolist() == bits(t0).tolist()
    # a stale array would show: the weights and chi2 that come back are those at the returned poses, not all 1, and (where the poses moved)
    # far from those of the start
    here = P.edge_terms(a["R"], a["t"], g["src"], g["tgt"], g["Rz"], g["tz"], g["info"], g["uncertain"], g["mu"])
    assert bits(a["w"]).tolist() == bits(here["w"]).tolist() and bits(a["chi2"]).tolist() == bits(here["chi2"]).tolist()
    assert (np.abs(a["w"] - 1.0) > 1e-6).sum() >= 5                                            # (six decades above the GPU suite's 1e-12)
    if accepted:
        assert np.abs(a["w"] - at_start["w"]).max() > 1e-3 and np.abs(a["chi2"] - at_start["chi2"]).max() > 1e-3


@pytest.mark.parametrize("name", SOLVE_GRAPHS)
def test_capped_solves_run_to_their_cap(name):
    for cap in S.SOLVE_CAPS:
        (x, it, trace), (x2, it2, _) = S.solve_run(name, 0.0, cap), S.solve_run(name, 0.0, cap, True)
        spread = S.solve_spread(name, 0.0, cap)
        print("%-10s cap %2d: |r| / |g| = %.3e, max |x| %.3e, two orders %.3g" % (name, cap, trace[-1], np.abs(x).max(), spread))
        assert it == it2 == cap == len(trace) and trace[-1] > 1e-6                      # far from any stop of its own
        assert within_a_decade(spread, SOLVE_SPREAD[(name, "cap", cap)])
    assert {c % S.SYNC_EVERY for c in S.SOLVE_CAPS} >= {0, 1, S.SYNC_EVERY - 1} and max(S.SOLVE_CAPS) > 2 * S.SYNC_EVERY > min(S.SOLVE_CAPS)


@pytest.mark.parametrize("name", SOLVE_GRAPHS)
def test_the_loose_solves_end_inside_a_chunk(name):
    tol, cap = S.LOOSE
    chunks = []
    for lam in S.LOOSE_LAMBDAS:
        (x, it, trace), (_, it2, trace2) = S.solve_run(name, tol, cap, False, lam), S.solve_run(name, tol, cap, True, lam)
        spread = S.solve_spread(name, tol, cap, lam)
        print("%-10s tolerance %g, lambda %g: %d iterations, |r| / |g| ... %s, two orders %.3g" % (name, tol, lam, it, " ".join("%.3g" % v for v in trace[-3:]), spread))
        assert it == it2 and 1 < it % S.SYNC_EVERY < S.SYNC_EVERY - 1 and cap > 10 * S.SYNC_EVERY   # iterations of the same chunk are enqueued behind the stop
        assert all(abs(v - tol) > 0.01 * tol for v in trace + trace2) and trace[-1] <= tol < min(trace[:-1])
        assert within_a_decade(spread, SOLVE_SPREAD[(name, "loose", lam)])
        chunks.append(it // S.SYNC_EVERY)
    assert chunks == [0, 1]                                                                # the first chunk, and the second


@pytest.mark.parametrize("name", SOLVE_GRAPHS)
def test_a_tolerance_of_one_is_met_at_the_start(name):
    for tol in (1.0, 3.0):
        x, it, trace = S.solve_run(name, tol, 200)
        assert it == 0 and trace == () and not x.any()


def sorted_by_low_bits(nodes_of_entries, bits):
    """would a stable sort on the low `bits` bits of the node leave the list entries ordered by node?"""
    order = np.argsort(nodes_of_entries & ((1 << bits) - 1), kind="stable")
    return bool((np.diff(nodes_of_entries[order]) >= 0).all())


@pytest.mark.parametrize("V,bits", list(zip(S.SORT_BITS_V, (10, 20, 20, 30, 30))))
def test_sort_bits_cases(V, bits):
    g = S.system_graph(("sort_bits", V))
    assert S.sort_bits(V) == bits and len(g["R"]) == V and len(g["src"]) == S.SPARSE_EDGES
    nodes = g["nodes"]
    assert np.array_equal(nodes, P.used_nodes(g["src"], g["tgt"])) and len(nodes) == S.SPARSE_USED and g["ref"] in nodes
    assert {k for k in (0, 1023, 1024, (1 << 20) - 1, 1 << 20, V - 1) if k < V} <= set(nodes.tolist())
    entries = np.stack([g["src"], g["tgt"]], axis=1).reshape(-1).astype(np.int64)               # entry 2 e + side
    assert sorted_by_low_bits(entries, bits)
    if bits > 10:
        assert not sorted_by_low_bits(entries, bits - 10)                                      # ten bits fewer would not sort this graph
    assert np.bincount(np.searchsorted(nodes, entries)).max() <= S.LONG_LIST
    # the compacted restatement: against the dense one where that is cheap
    if V <= 1025:
        t = g["terms"]
        D, grad = P.node_blocks(V, g["src"], g["tgt"], t["M"], t["h"])
        isolated = np.setdiff1d(np.arange(V), nodes)
        assert np.array_equal(D[nodes], g["D"]) and np.array_equal(grad[nodes], g["g"]) and not D[isolated].any() and not grad[isolated].any()
        q = P.apply_system(g["src"], g["tgt"], t["M"], D, 1e-3, g["p"], g["ref"])
        assert np.array_equal(q, S.product(g, 1e-3, g["p"])) and not q[isolated].any() and not q[g["ref"]].any()


def test_the_wide_graph_leaves_the_small_paths():
    g = S.system_graph("wide")
    V, E = len(g["R"]), len(g["src"])
    assert (V, E) == (S.WIDE_V, S.WIDE_E) and (g["src"] != g["tgt"]).all()
    assert 2 * E > S.SORT_ONE_PASS                                                             # the radix sort's many-workgroup path
    assert S.pg_blocks(V) == 258 > S.ONE_TRIP[2] and S.pg_blocks(E) == 513 > S.ONE_TRIP[1]     # a second and a third trip per lane
    assert S.pg_blocks(V) > 2 * S.ONE_TRIP[2] and S.pg_blocks(E) > 2 * S.ONE_TRIP[1]
    degree = np.bincount(np.concatenate([g["src"], g["tgt"]]), minlength=V)
    assert degree[S.HUB] == S.HUB_DEGREE == 64 * 64 + 1 and degree.min() >= 1                  # 65 trips of the wave, the last with one lane
    assert (np.delete(degree, S.HUB) <= S.LONG_LIST).all() and S.sort_bits(V) == 20
    sides = np.flatnonzero((g["src"] == S.HUB) | (g["tgt"] == S.HUB))
    assert 1000 < (g["src"][sides] == S.HUB).sum() < 3000 and sides.max() - sides.min() > E // 2   # both signs, all along the list
    c = S.wide_consistent()
    assert np.abs(P.residuals(c["R"], c["t"], c["src"], c["tgt"], c["Rz"], c["tz"])).max() <= 1e-12


def test_the_zero_edge_is_zero_in_the_restatement():
    g = S.system_graph("zero_edge")
    t = g["terms"]
    assert not t["r"][0].any() and t["chi2"][0] == 0.0 and t["w"][0] == 1.0 and g["uncertain"][0] == 1 and g["mu"] > 0
    assert np.isfinite(t["M"][0]).all() and not t["h"][0].any() and t["r"][1].any()
