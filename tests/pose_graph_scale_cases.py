"""The cases of tests/test_gpu_pose_graph_scale.py and what they share: the runs at which mi_pose_graph_optimize leaves the happy path of
its Levenberg-Marquardt loop (rejected steps, MI_STOP_ERROR_INCREASED, MI_STOP_MAX_ITERATIONS, no linearisation beyond the first, an inner
solve of no iterations), the inner solves that end at their cap or inside an enqueued chunk of PG_SYNC_EVERY iterations, and the graphs at
which mi_pose_graph_system leaves its small paths: every width of the incidence sort's keys, more list entries than the radix sort's
one-workgroup path holds, more partial rows than reduce_partials takes in one trip, a hub of 4 097 entries.
tests/test_pose_graph_scale_cases.py holds every case to its name with tests/pose_graph_reference.py alone.

Every case is cached, seeded and frozen; its users leave it unchanged.  No tolerance is introduced here."""
import functools

import numpy as np

import pose_graph_reference as P

SYNC_EVERY = 16                      # PG_SYNC_EVERY (csrc/pose_graph_api.hip): inner iterations enqueued between two reads of the state
MAX_REJECTIONS = 8                   # PG_MAX_REJECTIONS
LAMBDA_MIN = 1e-12                   # PG_LAMBDA_MIN
LONG_LIST = 64                       # PG_LONG_LIST (csrc/pose_graph_terms.hpp): a longer list is summed by one wave
SORT_ONE_PASS = 4096 * 64            # keys up to which the library's radix sort takes its one-workgroup path (tests/search_scale_cases.py)
BLOCK = 256                          # lanes of a workgroup: pg_blocks(n) partial rows
ONE_TRIP = {1: 256, 2: 128}          # reduce_partials<W> (csrc/reduce.hpp): rows that its 256 / W row groups take in one trip


def frozen(a):
    if isinstance(a, np.ndarray):
        a.setflags(write=False)
    return a


def frozen_dict(d):
    return {k: frozen(v) for k, v in d.items()}


def pg_blocks(n):
    return (n + BLOCK - 1) // BLOCK


def sort_bits(V):
    """pg_setup's rule: the key bits of the incidence sort, 10, 20 or 30 -- the first of them that holds node V - 1."""
    bits = 10
    while bits < 30 and (1 << bits) < V:
        bits += 10
    return bits


def edge_order(E, seed=5):
    """the second order of the edges in which the restatement runs: another order of every sum over the edges and over a node's list"""
    return np.random.default_rng(seed).permutation(E)


# ---- A. the outer loop
@functools.lru_cache(maxsize=None)
def loop_graph():
    """The 60-node ring with 20 loop edges, every measurement 0.02 off (so the cost does not end at 0 and chi2 and w stay visible), three
    edges in ten uncertain under mu = 20."""
    g = P.consistent_graph("ring60", 1)
    rng = np.random.default_rng(1001)
    E = len(g["src"])
    g["Rz"], g["tz"] = P.update(g["Rz"], g["tz"], 0.02 * rng.normal(size=(E, 6)))
    g["uncertain"] = (rng.uniform(size=E) < 0.3).astype(np.uint8)
    g["mu"] = 20.0
    return frozen_dict(g)


# name -> (perturbation of the start, its seed, the parameters).  Chosen on the CPU so that no decision of the restatement is a near tie
# (tests/test_pose_graph_scale_cases.py); the inner caps are small, which makes steps inexact and the runs cheap, and 20 and 40 end a solve
# in the middle of an enqueued chunk.
LOOP = {
    "rejected_then_accepted": (0.6, 9, dict(max_pcg_iterations=40, absolute_cost=10.0)),
    "error_increased_at_once": (1.0, 7, dict(max_pcg_iterations=48, lambda0=1e-12)),
    "error_increased_after_accepting": (0.6, 9, dict(max_pcg_iterations=20, absolute_cost=10.0)),
    "max_iterations_1": (0.2, 7, dict(max_pcg_iterations=100, max_iterations=1)),
    "max_iterations_3": (0.6, 9, dict(max_pcg_iterations=80, max_iterations=3)),
    "max_iterations_0": (0.6, 9, dict(max_iterations=0)),
    "no_inner_iterations": (0.6, 9, dict(max_pcg_iterations=0)),
}


def loop_params(name):
    return dict(LOOP[name][2], line_process_mu=loop_graph()["mu"])


@functools.lru_cache(maxsize=None)
def loop_start(name):
    g = loop_graph()
    pert, seed, _ = LOOP[name]
    return tuple(frozen(a) for a in P.perturbed(np.random.default_rng(seed), g["R"], g["t"], pert))


@functools.lru_cache(maxsize=None)
def loop_run(name, permuted=False):
    """The restatement's run of a case with its edges as given or in edge_order: dict(R, t, w, chi2, report, trace), w and chi2 in the
    edges' own order either way."""
    g = loop_graph()
    R0, t0 = loop_start(name)
    E = len(g["src"])
    o = edge_order(E) if permuted else np.arange(E)
    trace = []
    out = P.optimize(R0, t0, g["src"][o], g["tgt"][o], g["Rz"][o], g["tz"][o], g["info"][o], g["uncertain"][o], solver="pcg", trace=trace, **loop_params(name))
    back = np.argsort(o)
    out["w"], out["chi2"], out["trace"] = out["w"][back], out["chi2"][back], tuple(trace)
    return frozen_dict(out)


def decisions(run):
    """what must not depend on roundoff: the trials' outcomes and inner iterations, and the report's integers and lambda"""
    rep = run["report"]
    return tuple((r["accepted"], r["inner"], r["lam"]) for r in run["trace"]), rep[2], rep[3], rep[4], rep[5], rep[6]


def loop_spread(name):
    """-> (relative cost, worst pose entry) between the restatement's two edge orders"""
    a, b = loop_run(name), loop_run(name, True)
    cost = abs(a["report"][1] - b["report"][1]) / a["report"][1]
    return cost, float(max(np.abs(a["R"] - b["R"]).max(), np.abs(a["t"] - b["t"]).max()))


# ---- B. the inner solve
SOLVE_LAMBDA = 1e-3
SOLVE_CAPS = (1, 15, 16, 17, 33)     # below, at and above one chunk, and into a third
LOOSE = (1e-2, 200)                  # a tolerance met inside an enqueued chunk of a solve whose cap is far:
LOOSE_LAMBDAS = (0.1, SOLVE_LAMBDA)  # inside the first chunk (9 and 10 iterations) and inside the second (25)


@functools.lru_cache(maxsize=None)
def system_graph(name):
    """The graphs of the per-element checks, as tests/test_gpu_pose_graph.py makes them: poses a few tenths of a radian off the measurements,
    three edges in ten uncertain under mu = 20, a random p, the restatement's terms (and, for the small graphs, its dense blocks)."""
    rng = np.random.default_rng(11)
    nodes = None
    if name == "ring60":                           # 60 + 20, two duplicate edges, and node 60 isolated
        V = 61
        src, tgt = P.ring_edges(rng, 60, 20)
        src, tgt, ref = np.concatenate([src, src[[3, 70]]]), np.concatenate([tgt, tgt[[3, 70]]]), 0
    elif name == "random300":
        V = 300
        (src, tgt), ref = P.random_graph_edges(rng, V, 100), 299
    elif name == "zero_edge":                      # edge 0 between two identity poses, measured as the identity; uncertain, so that w is computed
        V = 3
        src, tgt, ref = np.array([0, 1], np.int32), np.array([1, 2], np.int32), 2
    elif name == "wide":
        V = WIDE_V
        src, tgt = wide_edges(rng)
        ref = 17
    elif name[0] == "sort_bits":
        V = name[1]
        src, tgt, nodes = sparse_edges(rng, V)
        ref = int(nodes[len(nodes) // 2])
    else:
        raise ValueError(name)
    E = len(src)
    if nodes is None:
        R, t = P.random_poses(rng, V)
    else:                                          # the isolated nodes: one pose repeated
        one = P.random_poses(rng, 1)
        R, t = np.tile(one[0], (V, 1, 1)), np.tile(one[1], (V, 1))
        R[nodes], t[nodes] = P.random_poses(rng, len(nodes))
    if name == "zero_edge":
        R[:2], t[:2] = np.eye(3), 0.0
    Rz, tz = P.measure(R, t, src, tgt)
    true_Z = (Rz, tz)
    Rz, tz = P.update(Rz, tz, np.concatenate([0.2 * rng.normal(size=(E, 3)), 0.3 * rng.normal(size=(E, 3))], axis=1))
    uncertain = (rng.uniform(size=E) < 0.3).astype(np.uint8)
    if name == "zero_edge":
        Rz[0], tz[0], uncertain[0] = np.eye(3), 0.0, 1
    g = dict(R=R, t=t, src=src.astype(np.int32), tgt=tgt.astype(np.int32), Rz=Rz, tz=tz, info=P.random_information(rng, E), uncertain=uncertain, ref=ref,
             mu=20.0, p=rng.normal(size=(V, 6)), nodes=nodes, true_Rz=true_Z[0], true_tz=true_Z[1])
    terms = P.edge_terms(R, t, g["src"], g["tgt"], Rz, tz, g["info"], uncertain, g["mu"])
    assert np.linalg.norm(terms["r"][:, :3], axis=1).max() < 2.5
    g["terms"] = frozen_dict(terms)
    # with nodes: the rows of the used nodes alone (P.node_blocks); every other node's are 0
    g["D"], g["g"] = P.node_blocks(V, g["src"], g["tgt"], terms["M"], terms["h"], nodes=nodes)
    return frozen_dict(g)


def product(g, lam, p):
    """the restatement's (H + lam diag H) p of a system graph, [V, 6]"""
    return P.apply_system(g["src"], g["tgt"], g["terms"]["M"], g["D"], lam, p, g["ref"], nodes=g["nodes"])


@functools.lru_cache(maxsize=None)
def solve_run(name, tolerance, cap, permuted=False, lam=SOLVE_LAMBDA):
    """The restatement's inner solve of system_graph(name) at lam, its edges as given or in edge_order -> (x, iterations, trace)"""
    g = system_graph(name)
    o = edge_order(len(g["src"])) if permuted else np.arange(len(g["src"]))
    M = g["terms"]["M"][o]
    D, grad = P.node_blocks(len(g["R"]), g["src"][o], g["tgt"][o], M, g["terms"]["h"][o])
    trace = []
    x, it, _ = P.pcg(g["src"][o], g["tgt"][o], M, D, grad, lam, g["ref"], tolerance, cap, trace=trace)
    return frozen(x), it, tuple(trace)


def solve_spread(name, tolerance, cap, lam=SOLVE_LAMBDA):
    """-> max |x - x'| / max |x| between the restatement's two edge orders"""
    a, b = solve_run(name, tolerance, cap, False, lam)[0], solve_run(name, tolerance, cap, True, lam)[0]
    return float(np.abs(a - b).max() / np.abs(a).max())


@functools.lru_cache(maxsize=None)
def compact_solve(name, lam, cap, permuted=False):
    """The restatement's inner solve, tolerance 0, of a system graph with isolated nodes, on its used nodes alone (relabelled in ascending
    order), its edges as given or in edge_order -> (x of the used nodes, iterations)"""
    g = system_graph(name)
    nodes = g["nodes"]
    o = edge_order(len(g["src"])) if permuted else np.arange(len(g["src"]))
    src, tgt, M = np.searchsorted(nodes, g["src"][o]), np.searchsorted(nodes, g["tgt"][o]), g["terms"]["M"][o]
    D, grad = P.node_blocks(len(nodes), src, tgt, M, g["terms"]["h"][o])
    x, it, _ = P.pcg(src, tgt, M, D, grad, lam, int(np.searchsorted(nodes, g["ref"])), 0.0, cap)
    return frozen(x), it


# ---- C. shapes
SORT_BITS_V = (1 << 10, (1 << 10) + 1, 1 << 20, (1 << 20) + 1, (1 << 20) + 3)
SPARSE_USED, SPARSE_EDGES = 300, 3000


def sparse_edges(rng, V):
    """SPARSE_EDGES edges among SPARSE_USED nodes of V, which always include 0, V - 1 and, where V allows, the nodes either side of 2^10 and
    of 2^20: a chain through the used nodes in a shuffled order, then random pairs.  -> src, tgt, the used nodes ascending"""
    forced = [k for k in (0, 1023, 1024, (1 << 20) - 1, 1 << 20, V - 1) if k < V]
    rest = np.setdiff1d(rng.choice(V, SPARSE_USED, replace=False), forced)[:SPARSE_USED - len(set(forced))]
    nodes = np.sort(np.concatenate([np.unique(forced), rest])).astype(np.int64)
    walk = rng.permutation(nodes)
    a, b = rng.choice(nodes, 2 * SPARSE_EDGES), rng.choice(nodes, 2 * SPARSE_EDGES)
    ok = a != b
    extra = SPARSE_EDGES - (len(nodes) - 1)
    src, tgt = np.concatenate([walk[:-1], a[ok][:extra]]).astype(np.int32), np.concatenate([walk[1:], b[ok][:extra]]).astype(np.int32)
    return src, tgt, nodes


WIDE_V, WIDE_E, HUB, HUB_DEGREE = 66000, 131100, 12345, 4097


def wide_edges(rng):
    """A chain through every node, random edges that leave the hub alone, and the hub's: HUB_DEGREE - 2 edges to distinct other nodes, their
    directions alternating, interleaved with the random ones."""
    spokes = np.setdiff1d(rng.choice(WIDE_V, HUB_DEGREE + 8, replace=False), [HUB - 1, HUB, HUB + 1])[:HUB_DEGREE - 2]
    flip = np.arange(len(spokes)) % 2 == 1
    count = WIDE_E - (WIDE_V - 1) - len(spokes)
    a, b = rng.integers(0, WIDE_V, 2 * count), rng.integers(0, WIDE_V, 2 * count)
    ok = (a != b) & (a != HUB) & (b != HUB)
    src = np.concatenate([a[ok][:count], np.where(flip, spokes, HUB)])
    tgt = np.concatenate([b[ok][:count], np.where(flip, HUB, spokes)])
    mix = rng.permutation(len(src))
    return (np.concatenate([np.arange(WIDE_V - 1), src[mix]]).astype(np.int32), np.concatenate([np.arange(1, WIDE_V), tgt[mix]]).astype(np.int32))


@functools.lru_cache(maxsize=None)
def wide_consistent(pert=0.05, seed=7):
    """the wide graph with the measurements made from its poses, and a start `pert` off them"""
    g = system_graph("wide")
    R0, t0 = P.perturbed(np.random.default_rng(seed), g["R"], g["t"], pert, ref=g["ref"])
    return frozen_dict(dict(R=g["R"], t=g["t"], src=g["src"], tgt=g["tgt"], Rz=g["true_Rz"], tz=g["true_tz"], info=g["info"], R0=R0, t0=t0, ref=g["ref"]))
