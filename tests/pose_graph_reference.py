"""The rules of mi_pose_graph_optimize (include/mi_slam.h) restated in numpy float64, edge-parallel, so that 5 000 nodes stay cheap: the
edge's error, residual, Jacobian and terms, the line process, the nodes' diagonal blocks and gradients, the Laplacian product, the stated
preconditioned conjugate gradients, the Levenberg-Marquardt loop with a dense or the stated inner solver -- and the graphs the CPU and GPU
tests share.  Sums are numpy's (np.add.at, in list order): the device's order of a node's sum moves bits, not the 1e-12 the tests hold it to.

Poses here are (R [V, 3, 3], t [V, 3]); to16 / from16 convert to the ABI's column-major 4 x 4."""
import numpy as np

LOG_SMALL = 1e-8
SERIES_BELOW = 1e-8
STOP_CONVERGED, STOP_MAX_ITERATIONS, STOP_ERROR_INCREASED = 1, 2, 4
DEFAULTS = dict(max_iterations=50, max_pcg_iterations=200, reference_node=0, pcg_tolerance=1e-8, relative_decrease=1e-9, absolute_cost=0.0,
                lambda0=1e-6, line_process_mu=0.0)
TRI = [(i, j) for i in range(6) for j in range(i, 6)]


def to16(R, t):
    T = np.zeros(R.shape[:-2] + (4, 4))
    T[..., :3, :3], T[..., :3, 3], T[..., 3, 3] = R, t, 1.0
    return np.ascontiguousarray(np.swapaxes(T, -1, -2)).reshape(R.shape[:-2] + (16,))


def from16(T16):
    T = np.swapaxes(np.asarray(T16, np.float64).reshape(T16.shape[:-1] + (4, 4)), -1, -2)
    return np.ascontiguousarray(T[..., :3, :3]), np.ascontiguousarray(T[..., :3, 3])


def skew(v):
    K = np.zeros(v.shape[:-1] + (3, 3))
    K[..., 0, 1], K[..., 0, 2], K[..., 1, 0], K[..., 1, 2], K[..., 2, 0], K[..., 2, 1] = -v[..., 2], v[..., 1], v[..., 2], -v[..., 0], -v[..., 1], v[..., 0]
    return K


def exp_so3(w):
    """Rodrigues as plane_solve.hpp states it: a = sin th / th, b = 2 sin^2(th / 2) / th^2, their series below 1e-8."""
    w = np.asarray(w, np.float64)
    th2 = (w * w).sum(axis=-1)
    th = np.sqrt(th2)
    small = th < SERIES_BELOW
    safe = np.where(small, 1.0, th)
    a = np.where(small, 1.0 - th2 / 6.0, np.sin(safe) / safe)
    b = np.where(small, 0.5 - th2 / 24.0, 2.0 * np.sin(0.5 * safe) ** 2 / np.where(small, 1.0, th2))
    K = skew(w)
    return np.eye(3) + a[..., None, None] * K + b[..., None, None] * (K @ K)


def log_so3(R):
    s = 0.5 * np.stack([R[..., 2, 1] - R[..., 1, 2], R[..., 0, 2] - R[..., 2, 0], R[..., 1, 0] - R[..., 0, 1]], axis=-1)
    n = np.sqrt((s * s).sum(axis=-1))
    c = 0.5 * (np.trace(R, axis1=-2, axis2=-1) - 1.0)
    small = n < LOG_SMALL
    k = np.where(small, 1.0, np.arctan2(n, c) / np.where(small, 1.0, n))
    return s * k[..., None]


def inverse(R, t):
    Ri = np.swapaxes(R, -1, -2)
    return Ri, -(Ri @ t[..., None])[..., 0]


def product(Ra, ta, Rb, tb):
    return Ra @ Rb, (Ra @ tb[..., None])[..., 0] + ta


def update(R, t, delta):
    """T <- exp(delta) T, delta = (omega, v)."""
    dR = exp_so3(delta[..., :3])
    return dR @ R, (dR @ t[..., None])[..., 0] + delta[..., 3:]


def measure(R, t, src, tgt):
    """Z_e = T_t^-1 T_s: what aligns the source scan to the target scan when the poses are (R, t)."""
    Ri, ti = inverse(R[tgt], t[tgt])
    return product(Ri, ti, R[src], t[src])


def residuals(R, t, src, tgt, Rz, tz):
    Ri, ti = inverse(R[tgt], t[tgt])
    Ra, ta = product(Ri, ti, R[src], t[src])
    Re, te = product(Ra, ta, *inverse(Rz, tz))
    return np.concatenate([log_so3(Re), te], axis=-1)


def adjoints(R, t, tgt):
    """A_e = Ad(T_t^-1) = [[Q, 0], [[t']x Q, Q]], Q = R_t^T, t' = -Q t_t."""
    Q, tp = inverse(R[tgt], t[tgt])
    A = np.zeros((len(tgt), 6, 6))
    A[:, :3, :3], A[:, 3:, 3:], A[:, 3:, :3] = Q, Q, skew(tp) @ Q
    return A


def symmetric(info):
    """Only the upper triangle of an information matrix is read."""
    info = np.asarray(info, np.float64).reshape(-1, 6, 6)
    up = np.triu(info)
    return up + np.swapaxes(np.triu(info, 1), -1, -2)


def line_process(chi2, uncertain, mu):
    on = (np.zeros(len(chi2), bool) if uncertain is None else np.asarray(uncertain).astype(bool)) & (mu > 0)
    d = np.where(on, mu + chi2, 1.0)
    return np.where(on, (mu / d) ** 2, 1.0), np.where(on, mu * chi2 / d, chi2)


def edge_terms(R, t, src, tgt, Rz, tz, info, uncertain=None, mu=0.0):
    L = symmetric(info)
    r = residuals(R, t, src, tgt, Rz, tz)
    u = (L @ r[..., None])[..., 0]
    chi2 = (r * u).sum(axis=-1)
    w, share = line_process(chi2, uncertain, mu)
    A = adjoints(R, t, tgt)
    At = np.swapaxes(A, -1, -2)
    M = w[:, None, None] * (At @ L @ A)
    h = w[:, None] * (At @ u[..., None])[..., 0]
    return dict(r=r, chi2=chi2, w=w, share=share, A=A, M=M, h=h, cost=float(share.sum()))


def used_nodes(src, tgt):
    """The nodes that some edge touches, ascending."""
    return np.unique(np.concatenate([np.asarray(src), np.asarray(tgt)]))


def node_blocks(V, src, tgt, M, h, nodes=None):
    """-> D [V, 6, 6], g [V, 6]; with nodes (used_nodes: ascending, every edge's ends among them) the rows of those nodes alone, in their
    order -- every other node's block and gradient are 0, and a node's sum depends on the edges' order only, not on the labels."""
    if nodes is not None:
        src, tgt, V = np.searchsorted(nodes, src), np.searchsorted(nodes, tgt), len(nodes)
    D, g = np.zeros((V, 6, 6)), np.zeros((V, 6))
    np.add.at(D, src, M); np.add.at(D, tgt, M)
    np.add.at(g, src, h); np.add.at(g, tgt, -h)
    return D, g


def apply_system(src, tgt, M, D, lam, p, ref, nodes=None):
    """(H + lam diag H) p in the Laplacian form, p_ref taken as 0 and the reference's row left 0.  With nodes (used_nodes) D holds the rows
    of those nodes alone (node_blocks with nodes); p and the result stay [V, 6], the rows of every other node 0."""
    if nodes is not None:
        at = np.searchsorted(nodes, ref)
        inner = apply_system(np.searchsorted(nodes, src), np.searchsorted(nodes, tgt), M, D, lam, p[nodes],
                             int(at) if at < len(nodes) and nodes[at] == ref else None)
        q = np.zeros_like(p)
        q[nodes] = inner
        return q
    p = p.copy()
    if ref is None:
        ref = []
    p[ref] = 0.0
    y = (M @ (p[src] - p[tgt])[..., None])[..., 0]
    q = np.zeros_like(p)
    np.add.at(q, src, y); np.add.at(q, tgt, -y)
    q += lam * np.diagonal(D, axis1=-2, axis2=-1) * p
    q[ref] = 0.0
    return q


def assemble(V, src, tgt, M):
    """H as a dense 6 V x 6 V matrix (a few hundred nodes at most)."""
    H = np.zeros((V, 6, V, 6))
    for e in range(len(src)):
        s, k = src[e], tgt[e]
        H[s, :, s, :] += M[e]; H[k, :, k, :] += M[e]
        H[s, :, k, :] -= M[e]; H[k, :, s, :] -= M[e]
    return H.reshape(6 * V, 6 * V)


def solve6(A, b):
    """plane_solve6's rule for A x = b, a batch of systems [V, 6, 6], [V, 6] -> x, ok: ok is False where it calls A degenerate (a diagonal
    entry <= 0 or not finite, or a pivot of the unit-diagonal scaling's LDL^T below 1e-10); x is undefined there."""
    d = np.diagonal(A, axis1=-2, axis2=-1)
    ok = (d > 0).all(axis=-1) & np.isfinite(d).all(axis=-1)
    s = 1.0 / np.sqrt(np.where(ok[:, None], d, 1.0))
    S = A * s[:, :, None] * s[:, None, :]
    Lm, piv = np.tile(np.eye(6), (len(A), 1, 1)), np.ones((len(A), 6))
    for j in range(6):
        pj = 1.0 - (Lm[:, j, :j] ** 2 * piv[:, :j]).sum(axis=-1)
        ok &= pj >= 1e-10
        piv[:, j] = np.where(ok, pj, 1.0)
        for i in range(j + 1, 6):
            Lm[:, i, j] = (S[:, i, j] - (Lm[:, i, :j] * Lm[:, j, :j] * piv[:, :j]).sum(axis=-1)) / piv[:, j]
    y = (b * s).copy()
    for i in range(6):
        y[:, i] -= (Lm[:, i, :i] * y[:, :i]).sum(axis=-1)
    y /= piv
    for i in range(5, -1, -1):
        y[:, i] -= (Lm[:, i + 1:, i] * y[:, i + 1:]).sum(axis=-1)
    return y * s, ok


def precondition(D, lam, r):
    """z_k = (D_k + lam diag D_k)^-1 r_k, or r_k where the block is degenerate."""
    Dl = D + lam * D * np.eye(6)
    with np.errstate(all="ignore"):
        x, ok = solve6(Dl, r)
    return np.where(ok[:, None], x, r)


def pcg(src, tgt, M, D, g, lam, ref, tolerance, max_iterations, trace=None):
    """The stated inner solve: zero start, block-Jacobi preconditioner, stop at |r| <= tolerance |g| or at the cap.  -> x, iterations, |r| / |g|
    trace: a list that receives |r| / |g| behind every iteration."""
    r = -g.copy()
    r[ref] = 0.0
    x = np.zeros_like(r)
    z = precondition(D, lam, r)
    p = z.copy()
    rz, gg = float((r * z).sum()), float((r * r).sum())
    rr, it = gg, 0
    if not gg > 0 or max_iterations <= 0 or not np.sqrt(gg) > tolerance * np.sqrt(gg):         # (r_0 = -g: a tolerance >= 1 is met at the start)
        return x, 0, 1.0 if gg > 0 else 0.0
    while True:
        q = apply_system(src, tgt, M, D, lam, p, ref)
        pq = float((p * q).sum())
        if not pq > 0:
            break
        alpha = rz / pq
        x += alpha * p
        r -= alpha * q
        z = precondition(D, lam, r)
        rz_new, rr = float((r * z).sum()), float((r * r).sum())
        it += 1
        if trace is not None:
            trace.append(float(np.sqrt(rr) / np.sqrt(gg)))
        if not np.sqrt(rr) > tolerance * np.sqrt(gg) or it >= max_iterations or not rz_new > 0:
            break
        p = z + (rz_new / rz) * p
        rz = rz_new
    return x, it, float(np.sqrt(rr) / np.sqrt(gg))


def solve_dense(V, src, tgt, M, g, lam, ref):
    H = assemble(V, src, tgt, M)
    H = H + lam * np.diag(np.diagonal(H))
    keep = np.ones(6 * V, bool)
    keep[6 * ref:6 * ref + 6] = False
    dead = np.diagonal(H) <= 0                       # a node without edges: nothing to solve for
    keep &= ~dead
    x = np.zeros(6 * V)
    x[keep] = np.linalg.solve(H[np.ix_(keep, keep)], -g.reshape(-1)[keep])
    return x.reshape(V, 6)


def optimize(R, t, src, tgt, Rz, tz, info, uncertain=None, solver="dense", trace=None, **kw):
    """The outer loop as mi_slam.h states it.  -> dict(R, t, w, chi2, report) with report = (initial cost, final cost, linearisations,
    accepted steps, inner iterations in total, final lambda, stop reason, the last solve's relative residual).  trace: a list that receives
    one record per trial step: dict(lam, F, F_new, accepted, inner) -- the lambda it was solved at, the cost before it, the candidate's
    cost, whether it was taken, and the inner solve's iterations."""
    p = dict(DEFAULTS, **kw)
    V, ref, mu = len(R), p["reference_node"], p["line_process_mu"]
    src, tgt = np.asarray(src), np.asarray(tgt)
    degree = np.bincount(np.concatenate([src, tgt]), minlength=V)
    lin = edge_terms(R, t, src, tgt, Rz, tz, info, uncertain, mu)
    F = F0 = lin["cost"]
    lam, linearisations, accepted, rejections, inner, rel, stop = p["lambda0"], 1, 0, 0, 0, 0.0, 0
    w, chi2 = lin["w"], lin["chi2"]
    if F <= p["absolute_cost"]:
        stop = STOP_CONVERGED
    elif p["max_iterations"] < 1:
        stop = STOP_MAX_ITERATIONS
    while not stop:
        D, g = node_blocks(V, src, tgt, lin["M"], lin["h"])
        if solver == "dense":
            x, it = solve_dense(V, src, tgt, lin["M"], g, lam, ref), 0
        else:
            x, it, rel = pcg(src, tgt, lin["M"], D, g, lam, ref, p["pcg_tolerance"], p["max_pcg_iterations"])
            inner += it
        x[ref] = 0.0
        x[degree == 0] = 0.0
        Rn, tn = update(R, t, x)
        still = ~x.any(axis=1)
        Rn[still], tn[still] = R[still], t[still]
        cand = edge_terms(Rn, tn, src, tgt, Rz, tz, info, uncertain, mu)
        if trace is not None:
            trace.append(dict(lam=lam, F=F, F_new=cand["cost"], accepted=bool(cand["cost"] < F), inner=it))
        if cand["cost"] < F:
            decrease = (F - cand["cost"]) / F
            R, t, F, lin = Rn, tn, cand["cost"], cand
            w, chi2 = cand["w"], cand["chi2"]
            accepted, rejections, lam = accepted + 1, 0, max(lam / 10.0, 1e-12)
            if decrease <= p["relative_decrease"] or F <= p["absolute_cost"]:
                stop = STOP_CONVERGED
            elif linearisations >= p["max_iterations"]:
                stop = STOP_MAX_ITERATIONS
            else:
                linearisations += 1
        else:
            rejections += 1
            if rejections >= 8:
                stop = STOP_ERROR_INCREASED
            else:
                lam *= 10.0
    return dict(R=R, t=t, w=w, chi2=chi2, report=(F0, F, linearisations, accepted, inner, lam, stop, rel))


# ---- the graphs of the tests
def random_poses(rng, V, spread=2.0, angle=1.0):
    """Rotations of about a radian, positions a few units from the origin (the update turns about the world origin: the lever arm of a far
    node couples its rotation to its translation and costs the inner solve iterations -- 320 to 590 at this spread, 770 to 1 600 at 10)."""
    R = exp_so3(angle * rng.normal(size=(V, 3)))
    return R, spread * rng.normal(size=(V, 3))


def random_information(rng, E):
    B = rng.normal(size=(E, 6, 6))
    return B @ np.swapaxes(B, -1, -2) + 6.0 * np.eye(6)


def perturbed(rng, R, t, pert, ref=0):
    """Node k != ref moved by exp of pert N(0, 1) rotation and 5 pert N(0, 1) translation."""
    d = np.concatenate([pert * rng.normal(size=(len(R), 3)), 5.0 * pert * rng.normal(size=(len(R), 3))], axis=1)
    d[ref] = 0.0
    Rn, tn = update(R, t, d)
    Rn[ref], tn[ref] = R[ref], t[ref]
    return Rn, tn


def ring_edges(rng, V, loops):
    src = list(range(V))
    tgt = [(k + 1) % V for k in range(V)]
    while len(src) < V + loops:
        a, b = rng.integers(0, V, 2)
        if abs(int(a) - int(b)) % V not in (0, 1, V - 1):
            src.append(int(a)); tgt.append(int(b))
    return np.array(src, np.int32), np.array(tgt, np.int32)


def star_edges(V):
    """Every node k >= 1 tied to node 0, the directions alternating."""
    k = np.arange(1, V, dtype=np.int32)
    odd = (k % 2).astype(bool)
    return np.where(odd, 0, k).astype(np.int32), np.where(odd, k, 0).astype(np.int32)


def random_graph_edges(rng, V, extra):
    """A chain through every node plus `extra` random edges."""
    a = rng.integers(0, V, 2 * extra + 16)
    b = rng.integers(0, V, 2 * extra + 16)
    ok = a != b
    src = np.concatenate([np.arange(V - 1), a[ok][:extra]]).astype(np.int32)
    tgt = np.concatenate([np.arange(1, V), b[ok][:extra]]).astype(np.int32)
    return src, tgt


def consistent_graph(kind, seed):
    """-> dict(R, t, src, tgt, Rz, tz, info): true poses and the measurements made from them.  kind: ring60 | star200 | random300 | random5000"""
    rng = np.random.default_rng(seed)
    if kind == "ring60":
        V = 60
        src, tgt = ring_edges(rng, V, 20)
    elif kind == "star200":
        V = 200
        src, tgt = star_edges(V)
    elif kind == "random300":
        V = 300
        src, tgt = random_graph_edges(rng, V, 100)
    elif kind == "random5000":
        V = 5000
        src, tgt = random_graph_edges(rng, V, 15000)
    else:
        raise ValueError(kind)
    R, t = random_poses(rng, V)
    Rz, tz = measure(R, t, src, tgt)
    return dict(R=R, t=t, src=src, tgt=tgt, Rz=Rz, tz=tz, info=random_information(rng, len(src)))


def noisy_ring(seed, V=60, loops=20, noise=0.01, planted=4, mu=20.0):
    """The ring with uncertain loop edges: every measurement noisy, `planted` of the loop edges replaced by gross errors.
    -> the graph, a start (the odometry chained from node 0), the uncertain flags and the planted edges' indices"""
    rng = np.random.default_rng(seed)
    src, tgt = ring_edges(rng, V, loops)
    R, t = random_poses(rng, V)
    Rz, tz = measure(R, t, src, tgt)
    E = len(src)
    d = np.concatenate([noise * rng.normal(size=(E, 3)), noise * rng.normal(size=(E, 3))], axis=1)
    Rz, tz = update(Rz, tz, d)
    bad = V + rng.choice(loops, planted, replace=False)
    Rz[bad], tz[bad] = update(Rz[bad], tz[bad], np.concatenate([rng.normal(size=(planted, 3)), 3.0 * rng.normal(size=(planted, 3))], axis=1))
    uncertain = np.zeros(E, np.uint8)
    uncertain[V:] = 1
    info = random_information(rng, E)
    # the start: T_{k+1} = T_k Z_k^-1 along the ring's first V - 1 edges (Z = T_t^-1 T_s, so T_t = T_s Z^-1)
    R0, t0 = R.copy(), t.copy()
    for k in range(V - 1):
        Zi = inverse(Rz[k], tz[k])
        R0[k + 1], t0[k + 1] = product(R0[k], t0[k], *Zi)
    return dict(R=R, t=t, src=src, tgt=tgt, Rz=Rz, tz=tz, info=info, R0=R0, t0=t0, uncertain=uncertain, planted=np.sort(bad), mu=mu)
