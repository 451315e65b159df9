"""The contract of mi_fgr_register (include/mi_slam.h) restated in numpy float64, rule by rule: the matches by rank, the tuple filter (the
draws and the edge rule are mi_ransac_register's: tests/ransac_reference.py), the used list, the scale and the schedule of mu, one
linearisation as the 32 sums -- in the library's own fixed summation order, beside math.fsum of the same terms -- the loop (the solve, the
update and the stop rule are mi_icp_plane_register's: tests/plane_reference.py) and the weights.

Matrices here are indexed [row, col]; the C interface's column-major 4 x 4 is capi's business."""
import math

import numpy as np

import plane_reference as P
import ransac_reference as RR

MAX_HYPOTHESES = 1 << 22
U = 2.0 ** -53
ONE_STAGE_ROWS, PARTS, GROUPS = 1024, 64, 8           # kernels.h: PLANE_ONE_STAGE_ROWS, PLANE_PARTS; reduce.hpp: 256 lanes / 32 sums


# ---- rules 1 and 2: the matches and the used list
def used_list(src, tgt, idx, tuple_scale=0.95, max_tuples=1000, tuple_trials=0, seed=0):
    """dict(used_src, used_tgt int [used], accepted: the trials that passed before max_tuples cuts, trials)"""
    idx = np.asarray(idx)
    i, s, t = RR.correspondences(src, tgt, idx)
    C, j = len(i), idx[i]
    if not np.float32(tuple_scale) > 0:
        return dict(used_src=i.astype(np.int32), used_tgt=j.astype(np.int32), accepted=0, trials=0)
    trials = int(tuple_trials) if tuple_trials > 0 else min(100 * C, MAX_HYPOTHESES)
    rk = RR.ranks(seed, 0, trials, C)
    distinct = (rk[:, 0] != rk[:, 1]) & (rk[:, 0] != rk[:, 2]) & (rk[:, 1] != rk[:, 2])
    ok, _ = RR.edge_rule(s[rk], t[rk], tuple_scale)
    accepted = np.flatnonzero(distinct & ok)
    ranks = rk[accepted[:max_tuples]].reshape(-1)
    return dict(used_src=i[ranks].astype(np.int32), used_tgt=j[ranks].astype(np.int32), accepted=len(accepted), trials=trials)


# ---- rule 3: the scale and the schedule
def diagonal2(cloud):
    c = np.ascontiguousarray(cloud, np.float32)
    d = c.max(axis=0).astype(np.float64) - c.min(axis=0).astype(np.float64)
    return float((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])


def scale2(src, tgt):
    return max(diagonal2(src), diagonal2(tgt))


def mu_at(D2, max_distance, division_factor, decrease_every, k):
    """mu of the linearisation that follows k applied updates"""
    mu = float(D2)
    delta2 = float(np.float32(max_distance)) * float(np.float32(max_distance))
    div = float(np.float32(division_factor))
    for _ in range(int(k) // int(decrease_every)):
        if mu > delta2:
            mu = mu / div
    return mu


# ---- rule 4: the terms of one linearisation
def residuals(p, q, R, t, c0, mu):
    """(u, r [used, 3], d2, w, l [used], finite [used]) of the used matches (p, q float64 [used, 3]) at the float64 pose (R, t)"""
    R, t, c0 = np.asarray(R, np.float64), np.asarray(t, np.float64), np.asarray(c0, np.float64)
    with np.errstate(all="ignore"):
        x = np.stack([((R[i, 0] * p[:, 0] + R[i, 1] * p[:, 1]) + R[i, 2] * p[:, 2]) + t[i] for i in range(3)], axis=1)
        finite = np.isfinite(x).all(axis=1)
        r, u = x - q, x - c0
        d2 = (r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2]
        w = mu / (mu + d2)
        l = w * w
    return u, r, d2, w, l, finite


def terms(p, q, R, t, c0, mu):
    """float64 [used, 32]: every used match's 30 entries in the row's layout (21 of H, 6 of g, e, aux, count, 0, 0); zeros where x is not finite"""
    u, r, d2, w, l, finite = residuals(p, q, R, t, c0, mu)
    n = len(p)
    zero, one = np.zeros(n), np.ones(n)
    Jx = [zero, u[:, 2], -u[:, 1], one, zero, zero]
    Jy = [-u[:, 2], zero, u[:, 0], zero, one, zero]
    Jz = [u[:, 1], -u[:, 0], zero, zero, zero, one]
    out = np.zeros((n, 32))
    with np.errstate(all="ignore"):
        k = 0
        for i in range(6):
            for j in range(i, 6):
                out[:, k] = l * ((Jx[i] * Jx[j] + Jy[i] * Jy[j]) + Jz[i] * Jz[j])
                k += 1
        for i in range(6):
            out[:, 21 + i] = l * ((Jx[i] * r[:, 0] + Jy[i] * r[:, 1]) + Jz[i] * r[:, 2])
        wm = w - 1.0
        out[:, 27] = l * d2 + mu * (wm * wm)
        out[:, 28] = d2
        out[:, 29] = 1.0
    out[~finite] = 0.0
    return out


# ---- the library's fixed summation order (reduce.hpp: wave_sum, reduce_partials; plane_kernels.hip: the slabs)
def _reduce_partials(rows):
    """one workgroup over [cnt, 32] rows: group g adds rows g, g + 8, .. in that order from 0, then the 8 groups are added in order from 0"""
    groups = np.zeros((GROUPS, rows.shape[1]))
    for b in range(len(rows)):
        groups[b % GROUPS] = groups[b % GROUPS] + rows[b]
    tot = np.zeros(rows.shape[1])
    for g in range(GROUPS):
        tot = tot + groups[g]
    return tot


def device_order_sums(T):
    """float64 [32]: the terms [used, 32] summed as the step and the reduce launches sum them"""
    used = len(T)
    nrows = (used + 63) // 64
    v = np.zeros((nrows * 64, T.shape[1]))
    v[:used] = T
    v = v.reshape(nrows, 64, T.shape[1])
    for off in (32, 16, 8, 4, 2, 1):
        v = v[:, :off] + v[:, off:2 * off]
    rows = v[:, 0]
    if nrows > ONE_STAGE_ROWS:
        per = (nrows + PARTS - 1) // PARTS
        rows = np.stack([_reduce_partials(rows[min(p * per, nrows):min(p * per + per, nrows)]) for p in range(PARTS)])
    return _reduce_partials(rows)


def tree_depth(used):
    """additions on the longest path from a term to its sum in device_order_sums (an addition to the 0 a partial sum starts from counts)"""
    nrows = (used + 63) // 64
    if nrows > ONE_STAGE_ROWS:
        per = (nrows + PARTS - 1) // PARTS
        return 6 + ((per + GROUPS - 1) // GROUPS + GROUPS) + (PARTS // GROUPS + GROUPS)
    return 6 + (nrows + GROUPS - 1) // GROUPS + GROUPS


def gamma(k):
    return k * U / (1.0 - k * U)


def matches(src, tgt, used):
    src, tgt = np.ascontiguousarray(src, np.float32), np.ascontiguousarray(tgt, np.float32)
    return src[used["used_src"]].astype(np.float64), tgt[used["used_tgt"]].astype(np.float64)


def system(src, tgt, used, R=None, t=None, mu=1.0):
    """One linearisation over the used list at the pose (R, t) (None: the identity) under mu -> dict(sums: in the library's order, fsum:
    math.fsum of the same terms, abs: the sums of their magnitudes, centre float32 [3], terms)"""
    R = np.eye(3) if R is None else R
    t = np.zeros(3) if t is None else t
    c0 = P.centre(tgt)
    p, q = matches(src, tgt, used)
    T = terms(p, q, R, t, c0.astype(np.float64), mu)
    with np.errstate(all="ignore"):
        return dict(sums=device_order_sums(T), fsum=np.array([math.fsum(T[:, k]) if np.isfinite(T[:, k]).all() else np.nan for k in range(32)]),
                    abs=np.abs(T).sum(axis=0), centre=c0, terms=T)


# ---- rules 5 and 6: the loop and the weights
def register(src, tgt, used, max_distance, division_factor=1.4, decrease_every=4, max_iterations=64, eps_rotation=0.0, eps_translation=0.0, init=None,
             reverse=False):
    """The whole loop over a used list -> dict(R, t float64, iterations, error float32, stop, final_mu float32, weights float32 [used]).
    reverse: the used list in the opposite order (the restatement's own sensitivity to the order of its sums)."""
    init = np.eye(4) if init is None else np.asarray(init, np.float32).astype(np.float64)
    R, t = init[:3, :3].copy(), init[:3, 3].copy()
    D2 = scale2(src, tgt)
    c0 = P.centre(tgt).astype(np.float64)
    p, q = matches(src, tgt, used)
    if reverse:
        p, q = p[::-1], q[::-1]
    iterations, error, last_k = 0, np.float32(0), 0
    stop = P.STOP_MAX_ITERATIONS if len(p) else P.STOP_NO_PAIRS
    while len(p) and iterations < max_iterations:
        last_k = iterations
        mu = mu_at(D2, max_distance, division_factor, decrease_every, iterations)
        sums = device_order_sums(terms(p, q, R, t, c0, mu))
        error = np.float32(sums[27] / sums[29]) if sums[29] > 0 else np.float32(0)
        if sums[29] < P.MIN_PAIRS:
            stop = P.STOP_NO_PAIRS
            break
        A, g = P.unpack_system(sums)
        x, _ = P.solve6(A, g)
        if x is None:
            stop = P.STOP_DEGENERATE
            break
        R, t = P.compose(P.rodrigues(x[:3]), x[3:], c0, R, t)
        iterations += 1
        if np.linalg.norm(x[:3]) <= np.float64(np.float32(eps_rotation)) and np.linalg.norm(x[3:]) <= np.float64(np.float32(eps_translation)):
            stop = P.STOP_CONVERGED
            break
        stop = P.STOP_MAX_ITERATIONS
    final_mu = mu_at(D2, max_distance, division_factor, decrease_every, last_k)
    weights = residuals(p, q, R, t, c0, final_mu)
    l = np.where(weights[5], weights[4], 0.0).astype(np.float32)
    return dict(R=R, t=t, iterations=iterations, error=error, stop=stop, final_mu=np.float32(final_mu), weights=l[::-1] if reverse else l)


# ---- the planted problems of the suites
def rotation(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def planted(C, outlier_share, seed, noise=0.002, angle=1.0, unmatched=0):
    """C matches in the unit cube: target = R0 source + t0 + noise, a rotation of `angle` rad about a random axis, t0 = (0.3, -0.2, 0.5); the
    share of wrong matches points at uniformly random places of the target's box; `unmatched` more source points have idx = -1.
    (src, tgt, idx, R0, t0, true [n])"""
    rng = np.random.default_rng(seed)
    n = C + unmatched
    src = rng.uniform(0, 1, (n, 3))
    R0, t0 = rotation(rng.normal(size=3), angle), np.array([0.3, -0.2, 0.5])
    tgt = src @ R0.T + t0 + noise * rng.normal(size=(n, 3))
    wrong = rng.permutation(C)[:int(round(outlier_share * C))]
    lo, hi = tgt.min(axis=0), tgt.max(axis=0)
    tgt[wrong] = rng.uniform(lo, hi, (len(wrong), 3))
    idx = np.arange(n, dtype=np.int32)
    idx[C:] = -1
    true = np.ones(n, bool)
    true[wrong] = False
    true[C:] = False
    return src.astype(np.float32), tgt.astype(np.float32), idx, R0, t0, true
