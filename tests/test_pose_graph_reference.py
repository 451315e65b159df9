"""CPU suite: tests/pose_graph_reference.py, the numpy float64 restatement of mi_pose_graph_optimize's rules, pinned to facts that do not
depend on it: zero residuals on measurements made from the poses, the Jacobians against central differences, the Laplacian product against
the assembled matrix, exp and log as inverses, convergence on consistent graphs from a perturbed start, the line process on planted
outliers, and its two inner solvers against each other.

NOISY_POSE_SPREAD and NOISY_COST_SPREAD are what the last test measured when it was written (seed 2, numpy 64-bit, the run of
test_dense_and_pcg_agree_on_the_noisy_ring: largest pose-entry difference 1.93e-12, relative cost difference 1.88e-16); the GPU suite's
bars on the noisy ring are taken from them (tests/test_gpu_pose_graph.py)."""
import functools

import numpy as np
import pytest

import pose_graph_reference as P

NOISY_SEED = 2
NOISY_POSE_SPREAD = 1.93e-12
NOISY_COST_SPREAD = 1.88e-16
CONSISTENT = (("ring60", 0.05), ("ring60", 0.2), ("star200", 0.1), ("random300", 0.1))


def start(g, pert, seed=7):
    return P.perturbed(np.random.default_rng(seed), g["R"], g["t"], pert)


@functools.lru_cache(maxsize=None)
def noisy_runs():
    n = P.noisy_ring(NOISY_SEED)
    kw = dict(line_process_mu=n["mu"], pcg_tolerance=1e-10, relative_decrease=1e-12)
    return n, {s: P.optimize(n["R0"], n["t0"], n["src"], n["tgt"], n["Rz"], n["tz"], n["info"], n["uncertain"], solver=s, **kw) for s in ("dense", "pcg")}


def test_measurements_made_from_the_poses_leave_nothing():
    g = P.consistent_graph("ring60", 1)
    o = P.edge_terms(g["R"], g["t"], g["src"], g["tgt"], g["Rz"], g["tz"], g["info"])
    D, grad = P.node_blocks(60, g["src"], g["tgt"], o["M"], o["h"])
    assert np.abs(o["r"]).max() <= 1e-13 and np.abs(grad).max() <= 1e-10 and o["cost"] <= 1e-24


def test_the_jacobians_match_central_differences():
    g = P.consistent_graph("ring60", 1)
    src, tgt = g["src"][:12], g["tgt"][:12]
    A = P.adjoints(g["R"], g["t"], tgt)
    step = 1e-6
    for side, sign in ((src, 1.0), (tgt, -1.0)):
        J = np.zeros((12, 6, 6))
        for c in range(6):
            r = []
            for s in (step, -step):
                R, t = g["R"].copy(), g["t"].copy()
                for e in range(12):               # one edge at a time: the ring's edges share nodes
                    d = np.zeros(6)
                    d[c] = s
                    Rk, tk = P.update(g["R"][side[e]], g["t"][side[e]], d)
                    R2, t2 = R.copy(), t.copy()
                    R2[side[e]], t2[side[e]] = Rk, tk
                    r.append(P.residuals(R2, t2, src[e:e + 1], tgt[e:e + 1], g["Rz"][e:e + 1], g["tz"][e:e + 1])[0])
            r = np.array(r).reshape(2, 12, 6)
            J[:, :, c] = (r[0] - r[1]) / (2 * step)
        assert np.abs(J - sign * A).max() <= 1e-6, np.abs(J - sign * A).max()


def test_the_laplacian_product_is_the_assembled_matrix():
    g = P.consistent_graph("ring60", 1)
    R0, t0 = start(g, 0.1)
    o = P.edge_terms(R0, t0, g["src"], g["tgt"], g["Rz"], g["tz"], g["info"])
    D, _ = P.node_blocks(60, g["src"], g["tgt"], o["M"], o["h"])
    H = P.assemble(60, g["src"], g["tgt"], o["M"])
    assert np.abs(H - H.T).max() <= 1e-12 * np.abs(H).max()
    rng = np.random.default_rng(3)
    for _ in range(3):
        p = rng.normal(size=(60, 6))
        p[0] = 0.0
        q = P.apply_system(g["src"], g["tgt"], o["M"], D, 0.0, p, 0)
        want = (H @ p.reshape(-1)).reshape(60, 6)
        want[0] = 0.0
        assert np.abs(q - want).max() <= 1e-12 * np.abs(want).max()
        assert float(p.reshape(-1) @ H @ p.reshape(-1)) >= 0.0
    # the diagonal blocks of the assembled matrix are the gathered ones
    for k in (0, 17, 59):
        assert np.abs(H[6 * k:6 * k + 6, 6 * k:6 * k + 6] - D[k]).max() <= 1e-12 * np.abs(D[k]).max()


def test_exp_and_log_are_inverses_up_to_three_radians():
    rng = np.random.default_rng(5)
    axis = rng.normal(size=(200, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    w = axis * np.concatenate([np.linspace(0.0, 3.0, 190), 10.0 ** -np.arange(4.0, 14.0)])[:, None]
    back = P.log_so3(P.exp_so3(w))
    assert np.abs(back - w).max() <= 1e-12, np.abs(back - w).max()          # (3 rad: sin is 0.14 there, the division costs one digit)


@pytest.mark.parametrize("kind,pert", CONSISTENT)
def test_consistent_graphs_converge_from_a_perturbed_start(kind, pert):
    g = P.consistent_graph(kind, 1)
    R0, t0 = start(g, pert)
    o = P.optimize(R0, t0, g["src"], g["tgt"], g["Rz"], g["tz"], g["info"], solver="dense", absolute_cost=1e-18)
    F0, F, linearisations, _, _, _, stop, _ = o["report"]
    err = max(np.abs(o["R"] - g["R"]).max(), np.abs(o["t"] - g["t"]).max())
    print("%s at %g: cost %.3g -> %.3g in %d linearisations, worst pose entry %.3g" % (kind, pert, F0, F, linearisations, err))
    assert stop == P.STOP_CONVERGED and linearisations <= 8 and err <= 1e-9 and F <= 1e-18


def test_the_line_process_switches_the_planted_edges_off():
    n, runs = noisy_runs()
    w = runs["dense"]["w"]
    planted = np.zeros(len(w), bool)
    planted[n["planted"]] = True
    print("planted weights %s, the others' smallest %.4f" % (w[planted], w[~planted].min()))
    assert (w[planted] < 0.25).all() and (w[~planted] > 0.9).all()
    assert (w[:60] == 1.0).all()                    # the odometry is not uncertain


def test_dense_and_pcg_agree_on_the_noisy_ring():
    _, runs = noisy_runs()
    a, b = runs["dense"], runs["pcg"]
    pose = max(np.abs(a["R"] - b["R"]).max(), np.abs(a["t"] - b["t"]).max())
    cost = abs(a["report"][1] - b["report"][1]) / a["report"][1]
    print("dense against pcg: poses %.3g, relative cost %.3g" % (pose, cost))
    assert a["report"][6] == b["report"][6] == P.STOP_CONVERGED
    # the constants are a record of this run; an order of magnitude around them is the same result on another BLAS
    assert pose <= 10 * NOISY_POSE_SPREAD and cost <= 10 * NOISY_COST_SPREAD + 1e-15
