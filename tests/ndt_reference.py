"""The restatement mi_ndt_constants, mi_ndt_voxels, mi_ndt_register and mi_ndt_system are tested against (numpy, CPU): the rules of
include/mi_slam.h retraced one by one, in the header's order of operations, vectorised over the points.  Built on tests/plane_reference.py
(the fp32 move, the solve, Rodrigues' formula, the composition) and tests/gicp_reference.py (the entries of H and g from a symmetric
matrix: NDT forms them from A = sum w M and b = sum w Md as generalized ICP forms them from M and Md).

A voxel map here is a dict(coord int32 [nv, 3], mean float32 [nv, 3], icov float32 [nv, 6], origin float32 [3], voxel float), the dict
cuda-slam_amd/capi.py's Context.ndt_voxels returns.  Matrices are [rows, 6], the upper triangle row by row: xx, xy, xz, yy, yz, zz."""
import numpy as np

import gicp_reference as G
import plane_reference as P

STOP_CONVERGED, STOP_MAX_ITERATIONS, STOP_NO_PAIRS, STOP_DEGENERATE = P.STOP_CONVERGED, P.STOP_MAX_ITERATIONS, P.STOP_NO_PAIRS, P.STOP_DEGENERATE
TRI = G.TRI
MAX_ABS = 1e18


def constants(voxel, outlier_ratio=0.55):
    """(d1, d2, h, k) float64 [4]: both arguments rounded to float32 first (they are floats in the C interface), then fp64 throughout"""
    r, o = np.float64(np.float32(voxel)), np.float64(np.float32(outlier_ratio))
    c1 = 10.0 * (1.0 - o)
    c2 = o / ((r * r) * r)
    d3 = -np.log(c2)
    d1 = -np.log(c1 + c2) - d3
    d2 = -2.0 * np.log((-np.log(c1 * np.exp(-0.5) + c2) - d3) / d1)
    return np.array([d1, d2, -0.5 * d2, -(d1 * d2)])


def voxel_index(p, origin, voxel):
    """(int64 [..., 3], ok [...]): floor((p - o) / v) in float32, mi_voxel_index's arithmetic; ok False where that function refuses"""
    p, o, v = np.asarray(p, np.float32), np.asarray(origin, np.float32), np.float32(voxel)
    with np.errstate(all="ignore"):
        q = np.floor((p - o) / v)
    ok = ((q >= np.float32(-2.0 ** 30)) & (q < np.float32(2.0 ** 30))).all(axis=-1)
    return np.where(ok[..., None], q, 0).astype(np.int64), ok


def voxels(cloud, voxel, origin=None, min_points=6, eig_ratio=0.01, mean=None):
    """mi_ndt_voxels -> dict(coord, count, mean, icov, cov: the outputs; origin, voxel; C float64 [rows, 6]: the covariance before the
    floor; C_abs: sum |term| / (count - 1) of every entry of C; lam [rows, 3]; M64, cov64: icov and cov before their rounding; has [rows]:
    the voxel has a distribution).  mean: the device's means, where the caller holds them (the scatter is taken about the OUTPUT mean, so
    that it can be retraced from the outputs whichever way the last bit of a mean fell)."""
    cloud = np.ascontiguousarray(cloud, np.float32)
    origin = cloud.min(axis=0) if origin is None else np.asarray(origin, np.float32)
    c, ok = voxel_index(cloud, origin, voxel)
    assert ok.all()
    order = np.lexsort((c[:, 0], c[:, 1], c[:, 2]))
    cs = c[order]
    head = np.ones(len(cs), bool)
    head[1:] = (cs[1:] != cs[:-1]).any(axis=1)
    start = np.flatnonzero(head)
    row_of = np.cumsum(head) - 1
    count = np.diff(np.append(start, len(cs))).astype(np.int32)
    p = cloud[order].astype(np.float64)
    if mean is None:
        mean = (np.add.reduceat(p, start, axis=0) / count[:, None]).astype(np.float32)
    mean = np.ascontiguousarray(mean, np.float32)
    d = p - mean.astype(np.float64)[row_of]
    prod = np.stack([d[:, a] * d[:, b] for a, b in TRI], axis=1)
    with np.errstate(all="ignore"):
        div = np.where(count > 1, count - 1, 1).astype(np.float64)[:, None]
        C = np.add.reduceat(prod, start, axis=0) / div
        C_abs = np.add.reduceat(np.abs(prod), start, axis=0) / div
    lam, V = np.linalg.eigh(G.full(C))
    has = (count >= min_points) & (lam[:, 2] > 0) & np.isfinite(lam[:, 2])
    floor = np.float64(np.float32(eig_ratio)) * lam[:, 2]
    lam2 = np.maximum(lam, floor[:, None])
    raised = (lam2 != lam).any(axis=1)
    with np.errstate(all="ignore"):
        M = np.einsum("nai,ni,nbi->nab", V, 1.0 / lam2, V)
        Cp = np.einsum("nai,ni,nbi->nab", V, lam2, V)
    M6 = np.stack([M[:, a, b] for a, b in TRI], axis=1)
    Cp6 = np.where(raised[:, None], np.stack([Cp[:, a, b] for a, b in TRI], axis=1), C)
    M6, Cp6 = np.where(has[:, None], M6, 0.0), np.where(has[:, None], Cp6, 0.0)
    return dict(coord=cs[start].astype(np.int32), count=count, mean=mean, icov=M6.astype(np.float32), cov=Cp6.astype(np.float32), origin=origin,
                voxel=float(voxel), C=C, C_abs=C_abs, lam=lam, lam_floored=lam2, raised=raised, M64=M6, cov64=Cp6, has=has)


def offsets(neighbourhood):
    """the (dx, dy, dz) of the lookups, in the header's order"""
    if neighbourhood == 1:
        return [(0, 0, 0)]
    if neighbourhood == 7:
        return [(0, 0, 0), (-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)]
    assert neighbourhood == 27
    return [(dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]


def has_distribution(vox):
    return (np.asarray(vox["icov"]) != 0).any(axis=1)


class Lookup:
    """the listed voxels with a distribution as a dictionary: rows(c) -> the row of every voxel coordinate c [k, 3], or -1"""

    def __init__(self, vox):
        rows = np.flatnonzero(has_distribution(vox))
        self.table = {tuple(int(v) for v in vox["coord"][r]): int(r) for r in rows}

    def rows(self, c):
        return np.array([self.table.get((int(x), int(y), int(z)), -1) for x, y, z in c], np.int64).reshape(len(c))


def centre(vox):
    has = has_distribution(vox)
    if not has.any():
        return np.zeros(3, np.float32)
    m = np.ascontiguousarray(vox["mean"], np.float32)[has]
    return np.float32(0.5) * (m.min(axis=0) + m.max(axis=0))


def h_entries(M, p):
    """the 21 entries of H = J^T M J (upper triangle, row-major) from M [k, 6] and p = P [k, 3]: gicp_reference.pair_terms' first 21"""
    return G.pair_terms(M, p, np.zeros_like(p))[:21]


def g_entries(b, p):
    b, p = [b[:, i] for i in range(3)], [p[:, i] for i in range(3)]
    return G.cross(p, b) + b


def term(q, mu, M, h, k):
    """the numbers of the terms (q_i, voxel_i), all float64 [n, ...]: dict(ok, d, Md, m, e, w)"""
    d = q - mu
    Md = np.stack([(G.sym(M, r, 0) * d[:, 0] + G.sym(M, r, 1) * d[:, 1]) + G.sym(M, r, 2) * d[:, 2] for r in range(3)], axis=1)
    m = (d[:, 0] * Md[:, 0] + d[:, 1] * Md[:, 1]) + d[:, 2] * Md[:, 2]
    ok = (M != 0).any(axis=1) & (m >= 0) & np.isfinite(m)
    with np.errstate(all="ignore"):
        e = np.exp(h * m)
    return dict(ok=ok, d=d, Md=Md, m=m, e=e, w=k * e)


def sums_at(q, vox, neighbourhood=7, outlier_ratio=0.55, lookup=None):
    """The sums of the moved points q (float32 [n, 3]) -> dict(sums float64 [32], abs float64 [32]: the sums of the magnitudes of every
    (point, voxel) term's own contribution, idx int32 [n], terms uint8 [n], centre float32 [3])."""
    q = np.ascontiguousarray(q, np.float32)
    n = len(q)
    lookup = lookup or Lookup(vox)
    _, _, h, k = constants(vox["voxel"], outlier_ratio)
    c0 = centre(vox)
    mean, icov = np.asarray(vox["mean"], np.float32).astype(np.float64), np.asarray(vox["icov"], np.float32).astype(np.float64)
    c, inside = voxel_index(q, vox["origin"], vox["voxel"])
    qd = q.astype(np.float64)
    Pq = qd - c0.astype(np.float64)
    A, b, E, terms = np.zeros((n, 6)), np.zeros((n, 3)), np.zeros(n), np.zeros(n, np.int64)
    idx = np.full(n, -1, np.int32)
    mags = np.zeros(32)
    for off in offsets(neighbourhood):
        rows = np.where(inside, lookup.rows(c + np.array(off)), -1)
        if off == (0, 0, 0):
            idx = rows.astype(np.int32)
        cand = np.flatnonzero(rows >= 0)
        if len(cand) == 0:
            continue
        M = icov[rows[cand]]
        t = term(qd[cand], mean[rows[cand]], M, h, k)
        use, ok = cand[t["ok"]], t["ok"]
        wM, wMd = t["w"][ok, None] * M[ok], t["w"][ok, None] * t["Md"][ok]
        A[use] += wM
        b[use] += wMd
        E[use] += t["e"][ok]
        terms[use] += 1
        for j, v in enumerate(h_entries(wM, Pq[use]) + g_entries(wMd, Pq[use]) + [t["e"][ok]]):
            mags[j] += np.abs(v).sum()
    live = np.flatnonzero(terms > 0)
    sums = np.zeros(32)
    for j, v in enumerate(h_entries(A[live], Pq[live]) + g_entries(b[live], Pq[live]) + [E[live]]):
        sums[j] = v.sum()
    sums[28] = mags[28] = float(len(live))
    sums[29] = mags[29] = float(terms.sum())
    return dict(sums=sums, abs=mags, idx=idx, terms=terms.astype(np.uint8), centre=c0, q=q)


def system(before, vox, R=None, t=None, neighbourhood=7, outlier_ratio=0.55, lookup=None):
    """One linearisation at the pose (R, t) (None: the identity): sums_at of q = the fp32 move of `before`"""
    R = np.eye(3) if R is None else R
    t = np.zeros(3) if t is None else t
    return sums_at(P.move_f32(R, t, before), vox, neighbourhood, outlier_ratio, lookup)


def step(before, vox, R, t, neighbourhood=7, outlier_ratio=0.55, lookup=None):
    """One iteration from the pose (R, t) -> dict(stop: None / STOP_NO_PAIRS / STOP_DEGENERATE, R, t: the pose behind it (unchanged on a
    stop), omega, v: the update's lengths, score: sum E / terms, system: the linearisation, kappa: cond(S) or inf)."""
    sy = system(before, vox, R, t, neighbourhood, outlier_ratio, lookup)
    sums = sy["sums"]
    out = dict(system=sy, R=np.array(R, np.float64), t=np.array(t, np.float64), omega=np.nan, v=np.nan, kappa=np.inf,
               score=np.float32(sums[27] / sums[29]) if sums[29] > 0 else np.float32(0))
    if sums[29] < P.MIN_PAIRS:
        return dict(out, stop=STOP_NO_PAIRS)
    A, g = P.unpack_system(sums)
    S, _ = P.scaled(A)
    if S is not None:
        out["kappa"] = float(np.linalg.cond(S))
    x, _ = P.solve6(A, g)
    if x is None:
        return dict(out, stop=STOP_DEGENERATE)
    Rn, tn = P.compose(P.rodrigues(x[:3]), x[3:], sy["centre"], out["R"], out["t"])
    return dict(out, stop=None, R=Rn, t=tn, omega=float(np.linalg.norm(x[:3])), v=float(np.linalg.norm(x[3:])))


def register(before, vox, eps_rotation=1e-6, eps_translation=1e-6, max_iterations=50, neighbourhood=7, outlier_ratio=0.55, init=None):
    """The whole loop -> dict(R, t float64, iterations, score float32, stop, poses: the fp64 pose before every iteration and the last one,
    steps: every iteration's step())."""
    init = np.eye(4) if init is None else np.asarray(init, np.float32).astype(np.float64)
    R, t = init[:3, :3].copy(), init[:3, 3].copy()
    lookup = Lookup(vox)
    poses, steps, iterations, score, stop = [(R, t)], [], 0, np.float32(0), STOP_MAX_ITERATIONS
    while iterations < max_iterations:
        s = step(before, vox, R, t, neighbourhood, outlier_ratio, lookup)
        steps.append(s)
        score = s["score"]
        if s["stop"] is not None:
            stop = s["stop"]
            break
        R, t = s["R"], s["t"]
        poses.append((R, t))
        iterations += 1
        if s["omega"] <= np.float64(np.float32(eps_rotation)) and s["v"] <= np.float64(np.float32(eps_translation)):
            stop = STOP_CONVERGED
            break
        stop = STOP_MAX_ITERATIONS
    return dict(R=R, t=t, iterations=iterations, score=score, stop=stop, poses=poses, steps=steps)
