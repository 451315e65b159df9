"""GPU suite of mi_pose_graph_optimize and mi_pose_graph_system against the float64 restatement of tests/pose_graph_reference.py.

The bounds (none of them taken from what the device gives):
  system       every output of one linearisation within 1e-12 max(1, max |ref|) over each edge's or node's own array: fp64 roundoff of
               1.1e-16 over a few hundred operations with two orders of margin.  H p for a random p the same, the reference's row 0.  The
               inner solve's x leaves |(H + lambda diag H) x + g| <= 10 pcg_tolerance |g|, formed in numpy from the restatement's blocks.
  same bits    two calls, and a call behind unrelated work on the context, give identical bytes; a hub's sums are the same bits from the
               one-lane and the one-wave path (zero-information padding edges move its list across the threshold of 64)
  optimisation consistent graphs: worst pose entry <= 1e-8 of the truth, MI_STOP_CONVERGED, <= 12 linearisations, at
               absolute_cost = 1e-18 F_initial.  The inner solve's cap is 2 000 there: the restatement's own PCG needs 320 to 590 iterations
               to 1e-8 on these graphs (tests/pose_graph_reference.py: random_poses), the default cap of 200 only shortens steps.
  noisy ring   against the restatement's dense run: the cost within 1 + max(10 x the recorded dense-against-pcg spread, 1e-9), the poses
               within max(10 x the recorded spread, 1e-9), the planted edges' weights < 0.25, all others > 0.9
Measured on an MI355X when the suite was written: DESIGN.md, "Pose-graph optimisation"."""
import ctypes as C
import functools

import numpy as np
import pytest

import pose_graph_reference as P
from test_pose_graph_reference import NOISY_COST_SPREAD, NOISY_POSE_SPREAD, NOISY_SEED

pytestmark = pytest.mark.gpu

BAR = 1e-12
TRI = P.TRI


def tri(M):
    return np.stack([M[:, i, j] for i, j in TRI], axis=1)


def T44(R, t):
    T = np.zeros((len(R), 4, 4))
    T[:, :3, :3], T[:, :3, 3], T[:, 3, 3] = R, t, 1.0
    return T


def split(T):
    return np.ascontiguousarray(T[:, :3, :3]), np.ascontiguousarray(T[:, :3, 3])


def with_start(g, pert, seed=7):
    g = dict(g)
    g["R0"], g["t0"] = P.perturbed(np.random.default_rng(seed), g["R"], g["t"], pert)
    return g


@functools.lru_cache(maxsize=None)
def system_graph(name):
    """The graphs of the per-element checks, at poses a few tenths of a radian off the measurements (residual angles below 2 rad)."""
    rng = np.random.default_rng(11)
    if name == "pair":
        R, t = P.random_poses(rng, 2)
        src, tgt, ref = np.array([0], np.int32), np.array([1], np.int32), 0
    elif name == "chain3":                         # the reference in the middle, one edge stored with source > target
        R, t = P.random_poses(rng, 3)
        src, tgt, ref = np.array([0, 2], np.int32), np.array([1, 1], np.int32), 1
    elif name == "ring60":                         # 60 + 20, two duplicate edges, and node 60 isolated
        R, t = P.random_poses(rng, 61)
        src, tgt = P.ring_edges(rng, 60, 20)
        src, tgt, ref = np.concatenate([src, src[[3, 70]]]), np.concatenate([tgt, tgt[[3, 70]]]), 0
    elif name == "star200":                        # the hub's list holds 199 entries: the one-wave path
        R, t = P.random_poses(rng, 200)
        (src, tgt), ref = P.star_edges(200), 5
    elif name == "random5000":                     # more than one workgroup in every kernel and every reduction
        R, t = P.random_poses(rng, 5000)
        (src, tgt), ref = P.random_graph_edges(rng, 5000, 15000), 4999
    else:
        raise ValueError(name)
    Rz, tz = P.measure(R, t, src, tgt)
    E = len(src)
    Rz, tz = P.update(Rz, tz, np.concatenate([0.2 * rng.normal(size=(E, 3)), 0.3 * rng.normal(size=(E, 3))], axis=1))
    uncertain = (rng.uniform(size=E) < 0.3).astype(np.uint8)
    g = dict(R=R, t=t, src=src.astype(np.int32), tgt=tgt.astype(np.int32), Rz=Rz, tz=tz, info=P.random_information(rng, E), uncertain=uncertain, ref=ref,
             mu=20.0, p=rng.normal(size=(len(R), 6)))
    ref_terms = P.edge_terms(R, t, g["src"], g["tgt"], Rz, tz, g["info"], uncertain, g["mu"])
    assert np.linalg.norm(ref_terms["r"][:, :3], axis=1).max() < 2.0
    g["terms"] = ref_terms
    g["D"], g["g"] = P.node_blocks(len(R), g["src"], g["tgt"], ref_terms["M"], ref_terms["h"])
    return g


def run_system(ctx, capi, g, solve=False, lambda0=1e-3, tol=1e-10, cap=5000, p=True):
    params = capi.pose_graph_params(reference_node=g["ref"], line_process_mu=g["mu"], lambda0=lambda0, pcg_tolerance=tol, max_pcg_iterations=cap)
    return ctx.pose_graph_system(T44(g["R"], g["t"]), g["src"], g["tgt"], T44(g["Rz"], g["tz"]), g["info"], g["uncertain"], params,
                                 p=g["p"] if p else None, solve=solve)


def ratio(dev, ref):
    """worst |dev - ref| / max(1, max |ref|) over each item's own array"""
    dev, ref = dev.reshape(len(ref), -1), ref.reshape(len(ref), -1)
    return float((np.abs(dev - ref).max(axis=1) / np.maximum(1.0, np.abs(ref).max(axis=1))).max())


@pytest.mark.parametrize("name", ["pair", "chain3", "ring60", "star200", "random5000"])
def test_system_per_element(ctx, capi, name):
    g = system_graph(name)
    lam = 1e-3
    o = run_system(ctx, capi, g, solve=True, lambda0=lam)
    t = g["terms"]
    want = dict(r=t["r"], chi2=t["chi2"], w=t["w"], M=tri(t["M"]), h=t["h"], diag=tri(g["D"]), g=g["g"],
                Hp=P.apply_system(g["src"], g["tgt"], t["M"], g["D"], lam, g["p"], g["ref"]))
    worst = {k: ratio(o[k], v) for k, v in want.items()}
    print("%s: worst |dev - ref| / max(1, max |ref|): %s" % (name, ", ".join("%s %.2e" % kv for kv in worst.items())))
    assert abs(o["cost"] - t["cost"]) <= BAR * max(1.0, t["cost"]) * len(g["src"])     # (a sum of E shares)
    assert (o["Hp"][g["ref"]] == 0.0).all()
    for k, v in worst.items():
        assert v <= BAR, (k, v)
    # the inner solve, held against the restatement's own blocks
    x = o["x"]
    assert (x[g["ref"]] == 0.0).all()
    rhs = -g["g"].copy()
    rhs[g["ref"]] = 0.0
    left = P.apply_system(g["src"], g["tgt"], t["M"], g["D"], lam, x, g["ref"]) - rhs
    rel = float(np.linalg.norm(left) / np.linalg.norm(rhs))
    print("%s: %d inner iterations, true |A x + g| / |g| = %.3e, the recurrence's %.3e" % (name, o["pcg_iterations"], rel, o["pcg_residual"]))
    assert rel <= 10 * 1e-10, rel


def outputs_bytes(o):
    return b"".join(np.ascontiguousarray(o[k]).tobytes() for k in sorted(o) if isinstance(o[k], np.ndarray))


def test_same_input_same_bits(ctx, capi):
    g = system_graph("star200")
    a = run_system(ctx, capi, g, solve=True)
    b = run_system(ctx, capi, g, solve=True)
    assert outputs_bytes(a) == outputs_bytes(b) and a["cost"] == b["cost"] and a["pcg_iterations"] == b["pcg_iterations"]
    # unrelated work on the context in between
    rng = np.random.default_rng(1)
    cloud = rng.uniform(-1, 1, (3000, 3)).astype(np.float32)
    ctx.knn_search(None, cloud, 4)
    normals = np.tile(np.array([0, 0, 1], np.float32), (3000, 1))
    ctx.icp_plane_register(cloud[::2] + np.float32(0.01), cloud, normals, capi.plane_params(max_iterations=3))
    c = run_system(ctx, capi, g, solve=True)
    assert outputs_bytes(a) == outputs_bytes(c)
    params = capi.pose_graph_params(reference_node=g["ref"], line_process_mu=g["mu"], max_iterations=3)
    args = (T44(g["R"], g["t"]), g["src"], g["tgt"], T44(g["Rz"], g["tz"]), g["info"], g["uncertain"], params)
    one, two = ctx.pose_graph_optimize(*args), ctx.pose_graph_optimize(*args)
    assert all(np.array_equal(x.view(np.uint64), y.view(np.uint64)) for x, y in zip(one[:3], two[:3])) and one[3] == two[3]


def test_a_hub_sums_to_the_same_bits_on_both_paths(ctx, capi):
    """Node 0 with 60 real edges; zero-information edges pad its list to 63 (one lane) and to 66 (one wave).  The padding adds exact zeros
    behind the real entries, so under the stated order the hub's block, gradient and row of H p must not move by a bit."""
    rng = np.random.default_rng(13)
    V = 80
    R, t = P.random_poses(rng, V)
    real_src, real_tgt = np.arange(1, 61, dtype=np.int32), np.zeros(60, np.int32)
    outs = {}
    for pad in (3, 6):
        src = np.concatenate([real_src, np.zeros(pad, np.int32)])
        tgt = np.concatenate([real_tgt, np.arange(61, 61 + pad, dtype=np.int32)])
        Rz, tz = P.measure(R, t, src, tgt)
        Rz, tz = P.update(Rz, tz, np.concatenate([0.2 * np.random.default_rng(14).normal(size=(len(src), 3)), 0.3 * np.random.default_rng(15).normal(size=(len(src), 3))], axis=1))
        info = P.random_information(np.random.default_rng(16), len(src))
        info[60:] = 0.0
        g = dict(R=R, t=t, src=src, tgt=tgt, Rz=Rz, tz=tz, info=info, uncertain=None, ref=79, mu=0.0, p=np.random.default_rng(17).normal(size=(V, 6)))
        outs[pad] = run_system(ctx, capi, g)
    for k in ("diag", "g", "Hp"):
        assert np.array_equal(outs[3][k][0].view(np.uint64), outs[6][k][0].view(np.uint64)), k
        assert np.abs(outs[3][k][0]).max() > 0


def optimise(ctx, capi, g, **kw):
    params = capi.pose_graph_params(**kw)
    poses, w, chi2, rep = ctx.pose_graph_optimize(T44(g["R0"], g["t0"]), g["src"], g["tgt"], T44(g["Rz"], g["tz"]), g["info"], g.get("uncertain"), params)
    return split(poses) + (w, chi2, rep)


@pytest.mark.parametrize("kind,pert", [("ring60", 0.05), ("ring60", 0.2), ("star200", 0.1), ("random300", 0.1), ("random5000", 0.1)])
def test_consistent_graphs_converge(ctx, capi, kind, pert):
    g = with_start(P.consistent_graph(kind, 1), pert)
    F0 = P.edge_terms(g["R0"], g["t0"], g["src"], g["tgt"], g["Rz"], g["tz"], g["info"])["cost"]
    R, t, w, chi2, rep = optimise(ctx, capi, g, absolute_cost=1e-18 * F0, max_pcg_iterations=2000)
    err = max(np.abs(R - g["R"]).max(), np.abs(t - g["t"]).max())
    print("%s at %g: %s, worst pose entry %.3g" % (kind, pert, rep, err))
    assert abs(rep["initial_cost"] - F0) <= 1e-12 * F0 * len(g["src"])
    assert rep["stop_reason"] == capi.STOP_CONVERGED and rep["linearisations"] <= 12 and err <= 1e-8
    assert (w == 1.0).all() and np.isfinite(chi2).all()


def test_noisy_ring_with_outliers(ctx, capi):
    n = P.noisy_ring(NOISY_SEED)
    kw = dict(line_process_mu=n["mu"], pcg_tolerance=1e-10, relative_decrease=1e-12)
    ref = P.optimize(n["R0"], n["t0"], n["src"], n["tgt"], n["Rz"], n["tz"], n["info"], n["uncertain"], solver="dense", **kw)
    R, t, w, chi2, rep = optimise(ctx, capi, n, **kw)
    pose = max(np.abs(R - ref["R"]).max(), np.abs(t - ref["t"]).max())
    print("noisy ring: %s; against the dense restatement: poses %.3g, cost %.17g against %.17g" % (rep, pose, rep["final_cost"], ref["report"][1]))
    assert rep["final_cost"] <= ref["report"][1] * (1.0 + max(10 * NOISY_COST_SPREAD, 1e-9))
    assert pose <= max(10 * NOISY_POSE_SPREAD, 1e-9)
    planted = np.zeros(len(w), bool)
    planted[n["planted"]] = True
    assert (w[planted] < 0.25).all() and (w[~planted] > 0.9).all()
    # chi2 and the weights belong together: w = (mu / (mu + chi2))^2 on the uncertain edges, 1 elsewhere, and the shares add up to the cost
    want_w, share = P.line_process(chi2, n["uncertain"], n["mu"])
    assert np.abs(w - want_w).max() <= 1e-15 and abs(share.sum() - rep["final_cost"]) <= 1e-12 * rep["final_cost"]


def test_gauge_and_degenerate_inputs(ctx, capi):
    g = with_start(P.consistent_graph("ring60", 1), 0.05)
    for ref in (0, 59):
        h = dict(g)
        h["R0"], h["t0"] = P.perturbed(np.random.default_rng(7), g["R"], g["t"], 0.05, ref=ref)
        R, t, _, _, rep = optimise(ctx, capi, h, reference_node=ref, max_pcg_iterations=2000)
        assert np.array_equal(R[ref].view(np.uint64), h["R0"][ref].view(np.uint64)) and np.array_equal(t[ref].view(np.uint64), h["t0"][ref].view(np.uint64))
        assert rep["accepted"] >= 1
    # no edge at all: the poses as given
    P0 = T44(g["R0"], g["t0"])
    out, w, chi2, rep = ctx.pose_graph_optimize(P0, np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros((0, 4, 4)), np.zeros((0, 6, 6)))
    assert np.array_equal(out, P0) and len(w) == 0 and rep["stop_reason"] == capi.STOP_CONVERGED and rep["linearisations"] == 0
    # an isolated node, and a component of three nodes without the reference
    rng = np.random.default_rng(21)
    Rt, tt = P.random_poses(rng, 64)
    src = np.concatenate([g["src"], [60, 61]]).astype(np.int32)
    tgt = np.concatenate([g["tgt"], [61, 62]]).astype(np.int32)
    Rt[:60], tt[:60] = g["R"], g["t"]
    Rz, tz = P.measure(Rt, tt, src, tgt)
    h = dict(R=Rt, t=tt, src=src, tgt=tgt, Rz=Rz, tz=tz, info=P.random_information(rng, len(src)))
    h["R0"], h["t0"] = P.perturbed(rng, Rt, tt, 0.05)
    F0 = P.edge_terms(h["R0"], h["t0"], src, tgt, Rz, tz, h["info"])["cost"]
    R, t, _, _, rep = optimise(ctx, capi, h, absolute_cost=1e-18 * F0, max_pcg_iterations=2000)
    assert np.array_equal(R[63], h["R0"][63]) and np.array_equal(t[63], h["t0"][63])
    assert np.isfinite(R).all() and np.isfinite(t).all() and rep["stop_reason"] == capi.STOP_CONVERGED
    r = P.residuals(R, t, src[-2:], tgt[-2:], Rz[-2:], tz[-2:])
    assert np.abs(r).max() <= 1e-8, np.abs(r).max()
    # a start at the solution: one linearisation, nothing accepted
    h = dict(g, R0=g["R"], t0=g["t"])
    R, t, _, _, rep = optimise(ctx, capi, h, absolute_cost=1e-20)
    assert rep["linearisations"] == 1 and rep["accepted"] == 0 and rep["stop_reason"] == capi.STOP_CONVERGED
    assert np.array_equal(R, g["R"]) and np.array_equal(t, g["t"])


def test_end_to_end_three_scans(ctx, capi):
    """Three views of one surface under known poses; the three pairwise point-to-plane registrations and their information matrices go
    in as edges as they come (float -> double and nothing else)."""
    rng = np.random.default_rng(31)
    xy = rng.uniform(-2, 2, (6000, 2))
    world = np.stack([xy[:, 0], xy[:, 1], 0.3 * np.sin(1.5 * xy[:, 0]) * np.cos(1.2 * xy[:, 1])], axis=1)
    nrm = np.stack([-0.45 * np.cos(1.5 * xy[:, 0]) * np.cos(1.2 * xy[:, 1]), 0.36 * np.sin(1.5 * xy[:, 0]) * np.sin(1.2 * xy[:, 1]), np.ones(6000)], axis=1)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    Rk = P.exp_so3(np.array([[0, 0, 0], [0.03, -0.02, 0.04], [-0.02, 0.03, -0.05]]))
    tk = np.array([[0, 0, 0], [0.05, -0.03, 0.02], [-0.04, 0.05, 0.03]])
    # scan 0 sees the whole surface, scan 1 its part x < 0.3 and scan 2 its part x > -0.3: scans 1 and 2 share a strip 0.6 wide only, so the
    # chain 0 <- 1 <- 2 hangs on the weakest of the three registrations, which the edge 2 -> 0 and the information matrices make up for
    x = xy[:, 0]
    picks = [rng.permutation(np.flatnonzero(keep))[:2000] for keep in (np.ones(6000, bool), x < 0.3, x > -0.3)]
    scans = [((world[p] - tk[k]) @ Rk[k]).astype(np.float32) for k, p in enumerate(picks)]          # T_k^-1 of the world points
    normals = [(nrm[p] @ Rk[k]).astype(np.float32) for k, p in enumerate(picks)]
    src, tgt, Z, info = [], [], [], []
    for s, k in ((1, 0), (2, 1), (2, 0)):
        R, t, _, _, why = ctx.icp_plane_register(scans[s], scans[k], normals[k], capi.plane_params(max_distance_squared=0.04))
        assert why in (capi.STOP_CONVERGED, capi.STOP_MAX_ITERATIONS), why
        T = np.eye(4, dtype=np.float32)
        T[:3, :3], T[:3, 3] = R, t
        _, _, I = ctx.evaluate_registration(scans[s], scans[k], T=T, max_d2=0.04)
        src.append(s); tgt.append(k); Z.append(T.astype(np.float64)); info.append(I)
    Z = np.array(Z)
    # the start: node 0 at the identity, node 1 from edge (1 -> 0), node 2 chained through node 1: T_s = T_t Z
    start = np.tile(np.eye(4), (3, 1, 1))
    start[1] = Z[0]
    start[2] = start[1] @ Z[1]
    truth = T44(Rk, tk)
    poses, w, chi2, rep = ctx.pose_graph_optimize(start, np.array(src, np.int32), np.array(tgt, np.int32), Z, np.array(info))
    before, after = np.abs(start - truth).max(), np.abs(poses - truth).max()
    print("three scans: %s; worst pose entry against the truth %.3g chained, %.3g optimised" % (rep, before, after))
    assert rep["final_cost"] <= rep["initial_cost"]
    assert after <= before + 1e-6


SENTINEL = -7.5


def refusal(ctx, capi, g, who="optimize", **change):
    """-> (rc, message, outputs untouched) of a call on graph g with one argument replaced"""
    a = dict(poses=P.to16(g["R"], g["t"]), src=g["src"].copy(), tgt=g["tgt"].copy(), Z=P.to16(g["Rz"], g["tz"]), info=g["info"].reshape(-1, 36).copy(),
             params=capi.pose_graph_params(), V=len(g["R"]), E=len(g["src"]))
    for k, v in change.items():
        if k in a:
            a[k] = v
        else:
            setattr(a["params"], k, v)
    V, E = len(g["R"]), len(g["src"])
    ptr = lambda x: None if x is None else x.ctypes.data
    if who == "optimize":
        outs = [np.full((V, 16), SENTINEL), np.full(E, SENTINEL), np.full(E, SENTINEL), np.full(8, SENTINEL)]
        rc = capi.pose_graph_optimize_raw(ctx._h, ptr(a["poses"]), a["V"], ptr(a["src"]), ptr(a["tgt"]), ptr(a["Z"]), ptr(a["info"]), None, a["E"],
                                          C.addressof(a["params"]), *[o.ctypes.data for o in outs])
    else:
        outs = [np.full(n, SENTINEL) for n in (6 * E, E, E, 21 * E, 6 * E, 21 * V, 6 * V, 6 * V, 6 * V, 2, 1)]
        rc = capi.pose_graph_system_raw(ctx._h, ptr(a["poses"]), a["V"], ptr(a["src"]), ptr(a["tgt"]), ptr(a["Z"]), ptr(a["info"]), None, a["E"],
                                        C.addressof(a["params"]), None, 1, *[o.ctypes.data for o in outs])
    return rc, capi.lib().mi_last_error().decode(), all((o == SENTINEL).all() for o in outs)


def edited(a, index, value):
    a = a.copy()
    a.reshape(-1)[index] = value
    return a


def test_refusals(ctx, capi):
    g = P.consistent_graph("ring60", 1)
    poses, Z, info = P.to16(g["R"], g["t"]), P.to16(g["Rz"], g["tz"]), g["info"].reshape(-1, 36)
    skewed = poses.copy()
    skewed[9, 0] += 0.01
    skewed[4, 5] += 0.01                              # two offenders: the lower index is named
    cases = [
        (dict(poses=None), "null poses"), (dict(V=0), "V = 0"), (dict(E=-1), "E = -1"), (dict(reference_node=60), "reference_node 60"),
        (dict(reference_node=-1), "reference_node -1"), (dict(src=edited(edited(g["src"], 30, 60), 7, -1)), "edge_source[7]"),
        (dict(tgt=edited(g["tgt"], 12, 60)), "edge_target[12]"), (dict(tgt=edited(g["tgt"], 5, g["src"][5])), "edge_target[5]"),
        (dict(poses=edited(edited(poses, 16 * 40 + 12, np.inf), 16 * 8 + 1, np.nan)), "poses[8]"),
        (dict(Z=edited(Z, 16 * 33 + 13, -np.inf)), "edge_T[33]"), (dict(info=edited(info, 36 * 21 + 4, np.nan)), "edge_information[21]"),
        (dict(poses=skewed), "poses[4]"), (dict(Z=edited(Z, 16 * 2 + 5, 1.5)), "edge_T[2]"),
        (dict(info=edited(edited(info, 36 * 50 + 7, -1.0), 36 * 9 + 35, -1e-3)), "edge_information[9]"),
        (dict(pcg_tolerance=float("nan")), "pcg_tolerance"), (dict(relative_decrease=-1.0), "relative_decrease"), (dict(absolute_cost=-1.0), "absolute_cost"),
        (dict(line_process_mu=float("nan")), "line_process_mu"), (dict(lambda0=0.0), "lambda0"), (dict(lambda0=-1.0), "lambda0"),
    ]
    for who in ("optimize", "system"):
        for change, needle in cases:
            rc, msg, untouched = refusal(ctx, capi, g, who, **change)
            assert rc == capi.MI_ERR_INVALID_ARG and msg.startswith("mi_pose_graph_%s: " % who) and needle in msg and untouched, (who, change.keys(), rc, msg, untouched)
    # a lower-triangle entry of an information matrix is not read
    rc, msg, _ = refusal(ctx, capi, g, info=edited(info, 36 * 3 + 6, np.nan))
    assert rc == capi.MI_OK, msg


def test_a_loaded_problem_survives(ctx, capi, bunny):
    before, after = bunny
    params = capi.icp_params(eps=1e-9, max_iterations=12)
    g = with_start(P.consistent_graph("star200", 1), 0.1)

    def icp(between):
        ctx.icp_load(before, after, params)
        ctx.icp_run(5)
        if between:
            run_system(ctx, capi, system_graph("star200"), solve=True)
            optimise(ctx, capi, g, max_iterations=3)
        ctx.icp_run(7)
        R, t, it, err, why = ctx.icp_result()
        return R.tobytes(), t.tobytes(), it, np.float32(err).tobytes(), why

    assert icp(True) == icp(False)
