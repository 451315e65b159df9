"""The restatement mi_estimate_color_gradients, mi_icp_color_register and mi_color_system are tested against (numpy, CPU): the rules of
include/mi_slam.h retraced one by one, every operation a rounded float64 operation in the stated order.  The neighbourhoods and the
matches are the keys of tests/knn_reference.py; the move, the centre, the solve, the update and the loop are tests/plane_reference.py's,
which the device shares between the two methods as well.

Matrices here are indexed [row, col]; the C interface's column-major 4 x 4 is capi's business."""
import numpy as np

import knn_reference as K
import plane_reference as P

LAMBDA = 0.968            # the authors' weight of the geometric term


def intensity_of_rgb(rgb):
    rgb = np.ascontiguousarray(rgb, np.float32)
    return ((rgb[:, 0] + rgb[:, 1]) + rgb[:, 2]) / np.float32(3)


def solve_gradient(M, b):
    """d = M^-1 b by the adjugate and the determinant, row-wise: M [r, 6] (xx, xy, xz, yy, yz, zz), b [r, 3] -> (d float64 [r, 3], zeros
    where det is <= 0 or not finite; det)"""
    M, b = np.asarray(M, np.float64), np.asarray(b, np.float64)
    m00, m01, m02, m11, m12, m22 = (M[:, i] for i in range(6))
    with np.errstate(all="ignore"):
        c00, c01, c02 = m11 * m22 - m12 * m12, m02 * m12 - m01 * m22, m01 * m12 - m02 * m11
        c11, c12, c22 = m00 * m22 - m02 * m02, m01 * m02 - m00 * m12, m00 * m11 - m01 * m01
        det = (m00 * c00 + m01 * c01) + m02 * c02
        ok = (det > 0) & np.isfinite(det)
        safe = np.where(ok, det, 1.0)
        d = np.stack([((c00 * b[:, 0] + c01 * b[:, 1]) + c02 * b[:, 2]) / safe,
                      ((c01 * b[:, 0] + c11 * b[:, 1]) + c12 * b[:, 2]) / safe,
                      ((c02 * b[:, 0] + c12 * b[:, 1]) + c22 * b[:, 2]) / safe], axis=1)
    d[~ok] = 0.0
    return d, det


def full3(M):
    """[r, 3, 3] symmetric from [r, 6]"""
    M = np.asarray(M, np.float64)
    return M[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(-1, 3, 3)


def cond1(M):
    """the 1-norm condition number of every symmetric 3 x 3 of M [r, 6]; inf where it is singular"""
    A = full3(M)
    out = np.full(len(A), np.inf)
    with np.errstate(all="ignore"):
        for i, a in enumerate(A):
            if np.isfinite(a).all() and np.linalg.det(a) != 0:
                out[i] = np.abs(a).sum(axis=0).max() * np.abs(np.linalg.inv(a)).sum(axis=0).max()
    return out


UPPER = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))


def normal_equations(n, e, delta, count):
    """(M [r, 6], b [r, 3]) of the tangent-plane least squares, the constraint included: n [r, 3] the normals, e [r, k, 3] the neighbours'
    offsets and delta [r, k] their intensity steps, nearest first, of which the first count [r] exist; all float64"""
    M, b = np.zeros((len(n), 6)), np.zeros((len(n), 3))
    for col in range(e.shape[1]):
        filled = col < count
        ec = e[:, col]
        s = (n[:, 0] * ec[:, 0] + n[:, 1] * ec[:, 1]) + n[:, 2] * ec[:, 2]
        u = ec - s[:, None] * n
        for slot, (a_, b_) in enumerate(UPPER):
            M[:, slot] = np.where(filled, M[:, slot] + u[:, a_] * u[:, b_], M[:, slot])
        for a_ in range(3):
            b[:, a_] = np.where(filled, b[:, a_] + u[:, a_] * delta[:, col], b[:, a_])
    w = np.asarray(count).astype(np.float64)
    ww = w * w
    for slot, (a_, b_) in enumerate(UPPER):
        M[:, slot] = M[:, slot] + (ww * n[:, a_]) * n[:, b_]
    return M, b


def gradients(cloud, normals, intensity, k, dist_mode=K.DIST_CPU_ROUNDING, max_d2=np.inf, only=None):
    """-> dict(grad float32 [r, 3], d float64 [r, 3]: before the rounding, count int32 [r], M float64 [r, 6]: the solved matrix, constraint
    included, b float64 [r, 3], solved bool [r]: neither of the three zero rules applied).  only: these rows alone."""
    cloud, normals = np.ascontiguousarray(cloud, np.float32), np.ascontiguousarray(normals, np.float32)
    intensity = np.ascontiguousarray(intensity, np.float32)
    rows = np.arange(len(cloud)) if only is None else np.asarray(only, np.int64)
    idx, _, count = K.unpack(K.sorted_keys(None, cloud, dist_mode, max_d2, keep=k, only=only), k)
    c64, I64 = cloud.astype(np.float64), intensity.astype(np.float64)
    p, n, Ii = c64[rows], normals[rows].astype(np.float64), I64[rows]
    j = np.where(np.arange(k)[None, :] < count[:, None], idx, 0)
    return solve_neighbourhoods(n, c64[j] - p[:, None, :], I64[j] - Ii[:, None], count)


def solve_neighbourhoods(n, e, delta, count):
    """gradients()' answer from the neighbourhoods themselves (normal_equations' arguments): the sums, the solve and the three zero rules"""
    M, b = normal_equations(n, e, delta, count)
    d, det = solve_gradient(M, b)
    usable = (np.asarray(count) >= 2) & (n != 0).any(axis=1)
    d[~usable] = 0.0
    solved = usable & (det > 0) & np.isfinite(det)
    return dict(grad=d.astype(np.float32), d=d, count=np.asarray(count, np.int32), M=M, b=b, solved=solved)


def pair_terms(q, a, c0, n, g, Ia, Ib):
    """(JG [r, 6], JC [r, 6], rG [r], rC [r]) of pairs, every argument float64"""
    dv, p = q - a, q - c0
    rG = (n[:, 0] * dv[:, 0] + n[:, 1] * dv[:, 1]) + n[:, 2] * dv[:, 2]
    cross = lambda y: [p[:, 1] * y[:, 2] - p[:, 2] * y[:, 1], p[:, 2] * y[:, 0] - p[:, 0] * y[:, 2], p[:, 0] * y[:, 1] - p[:, 1] * y[:, 0]]
    JG = np.stack(cross(n) + [n[:, 0], n[:, 1], n[:, 2]], axis=1)
    qp = dv - rG[:, None] * n
    rC = (((g[:, 0] * qp[:, 0] + g[:, 1] * qp[:, 1]) + g[:, 2] * qp[:, 2]) + Ia) - Ib
    gn = (g[:, 0] * n[:, 0] + g[:, 1] * n[:, 1]) + g[:, 2] * n[:, 2]
    mvec = g - gn[:, None] * n
    JC = np.stack(cross(mvec) + [mvec[:, 0], mvec[:, 1], mvec[:, 2]], axis=1)
    return JG, JC, rG, rC


def pair_entries(JG, JC, rG, rC, lam):
    """the 28 entries of every pair: 21 of H, 6 of g and e -> float64 [r, 28]"""
    lg = np.float64(np.float32(lam))
    lc = 1.0 - lg
    cols = [lg * (JG[:, a_] * JG[:, b_]) + lc * (JC[:, a_] * JC[:, b_]) for a_ in range(6) for b_ in range(a_, 6)]
    cols += [lg * (JG[:, a_] * rG) + lc * (JC[:, a_] * rC) for a_ in range(6)]
    cols += [lg * (rG * rG) + lc * (rC * rC)]
    return np.stack(cols, axis=1)


def sums_of_pairs(q, ib, after, normals, ia, grad, idx, d2, lam):
    """(sums float64 [32], the sums of the terms' magnitudes) of the pairs (i, idx[i]) with idx[i] >= 0, the moved points q and the
    matches' float32 distances d2 being given"""
    after, normals, grad = (np.ascontiguousarray(x, np.float32) for x in (after, normals, grad))
    pair = np.asarray(idx) >= 0
    jj = np.asarray(idx)[pair]
    c0 = P.centre(after).astype(np.float64)
    JG, JC, rG, rC = pair_terms(q[pair].astype(np.float64), after[jj].astype(np.float64), c0, normals[jj].astype(np.float64), grad[jj].astype(np.float64),
                                np.asarray(ia, np.float32)[jj].astype(np.float64), np.asarray(ib, np.float32)[pair].astype(np.float64))
    entries = pair_entries(JG, JC, rG, rC, lam)
    sums, mags = np.zeros(32), np.zeros(32)
    for k in range(28):           # (column by column, as plane_reference sums its terms: numpy's pairwise order along a contiguous vector)
        sums[k], mags[k] = np.ascontiguousarray(entries[:, k]).sum(), np.abs(np.ascontiguousarray(entries[:, k])).sum()
    d2p = np.asarray(d2)[pair].astype(np.float64)
    sums[28], mags[28] = d2p.sum(), np.abs(d2p).sum()
    sums[29] = mags[29] = float(pair.sum())
    return sums, mags


def system(before, ib, after, normals, ia, grad, R=None, t=None, dist_mode=K.DIST_CPU_ROUNDING, max_d2=np.inf, lam=LAMBDA, keys=None):
    """One linearisation at the pose (R, t) (None: the identity) -> dict(sums float64 [32], abs float64 [32]: the sums of the terms'
    magnitudes, idx int32 [n]: the fixed index of every pair or -1, centre float32 [3], q float32 [n, 3], d2 float32 [n], keys: the
    k = 1 keys of the moved points, which a second call at the same pose, mode and limit may hand back in)."""
    R = np.eye(3) if R is None else R
    t = np.zeros(3) if t is None else t
    after, normals = np.ascontiguousarray(after, np.float32), np.ascontiguousarray(normals, np.float32)
    q = P.move_f32(R, t, before)
    keys = K.sorted_keys(q, after, dist_mode, max_d2, keep=1) if keys is None else keys
    j, d2, count = K.unpack(keys, 1)
    j, d2 = j[:, 0], d2[:, 0]
    pair = (count == 1) & np.isfinite(d2)
    pair[pair] &= (normals[j[pair]] != 0).any(axis=1)
    idx = np.where(pair, j, -1).astype(np.int32)
    sums, mags = sums_of_pairs(q, ib, after, normals, ia, grad, idx, d2, lam)
    return dict(sums=sums, abs=mags, idx=idx, centre=P.centre(after), q=q, d2=d2, keys=keys)


def step(before, ib, after, normals, ia, grad, R, t, dist_mode=K.DIST_CPU_ROUNDING, max_d2=np.inf, lam=LAMBDA):
    """One iteration from the pose (R, t), as plane_reference.step: the same solve and update on this method's sums"""
    sy = system(before, ib, after, normals, ia, grad, R, t, dist_mode, max_d2, lam)
    sums = sy["sums"]
    out = dict(system=sy, R=np.array(R, np.float64), t=np.array(t, np.float64), omega=np.nan, v=np.nan, kappa=np.inf,
               error=np.float32(sums[27] / sums[29]) if sums[29] > 0 else np.float32(0))
    if sums[29] < P.MIN_PAIRS:
        return dict(out, stop=P.STOP_NO_PAIRS)
    A, g = P.unpack_system(sums)
    S, _ = P.scaled(A)
    if S is not None:
        out["kappa"] = float(np.linalg.cond(S))
    x, _ = P.solve6(A, g)
    if x is None:
        return dict(out, stop=P.STOP_DEGENERATE)
    Rn, tn = P.compose(P.rodrigues(x[:3]), x[3:], sy["centre"], out["R"], out["t"])
    return dict(out, stop=None, R=Rn, t=tn, omega=float(np.linalg.norm(x[:3])), v=float(np.linalg.norm(x[3:])))


def register(before, ib, after, normals, ia, grad, eps_rotation=1e-6, eps_translation=1e-6, max_iterations=50, max_d2=np.inf,
             dist_mode=K.DIST_CPU_ROUNDING, lam=LAMBDA, init=None):
    """The whole loop, as plane_reference.register -> dict(R, t float64, iterations, error float32, stop, poses, steps)."""
    init = np.eye(4) if init is None else np.asarray(init, np.float32).astype(np.float64)
    R, t = init[:3, :3].copy(), init[:3, 3].copy()
    poses, steps, iterations, error, stop = [(R, t)], [], 0, np.float32(0), P.STOP_MAX_ITERATIONS
    while iterations < max_iterations:
        s = step(before, ib, after, normals, ia, grad, R, t, dist_mode, max_d2, lam)
        steps.append(s)
        error = s["error"]
        if s["stop"] is not None:
            stop = s["stop"]
            break
        R, t = s["R"], s["t"]
        poses.append((R, t))
        iterations += 1
        if s["omega"] <= np.float64(np.float32(eps_rotation)) and s["v"] <= np.float64(np.float32(eps_translation)):
            stop = P.STOP_CONVERGED
            break
        stop = P.STOP_MAX_ITERATIONS
    return dict(R=R, t=t, iterations=iterations, error=error, stop=stop, poses=poses, steps=steps)


GRADIENT_LIMIT = 9.5          # max_distance_squared of the gradient scene: far beyond any k-list of the surface, short of the planted points' distance from it
GRADIENT_KS = (2, 8, 16, 32)
ILL_CONDITIONED = 1e8         # points whose cond_1(M) is beyond this are left out of the per-component bound ...
ILL_SHARE = 0.01              # ... and may be this share of a scene at most


def gradient_scene(name):
    """The fixed cloud of scene(name) with the planted cases behind it -> dict(cloud [4005, 3], normals, intensity, all float32; zero: the 40
    rows whose normal is (0, 0, 0); line: the four rows on a line of integer coordinates, alone within the limit, whose M is exactly
    singular; lonely: the row with no neighbour within the limit)."""
    s = scene(name)
    rng = np.random.default_rng(11)
    normals = s["normals"].copy()
    zero = np.sort(rng.permutation(4000)[:40])
    normals[zero] = 0
    up = np.array([0.0, 0.0, 1.0], np.float32)
    cloud = np.concatenate([s["fixed"], np.array([[20, 20, 0], [21, 20, 0], [22, 20, 0], [23, 20, 0], [-30, -30, 5]], np.float32)])
    normals = np.concatenate([normals, np.tile(up, (5, 1))])
    intensity = np.concatenate([s["ia"], np.array([0.1, 0.4, 0.2, 0.9, 0.5], np.float32)])
    return dict(cloud=frozen(cloud), normals=frozen(normals), intensity=frozen(intensity), zero=zero, line=np.arange(4000, 4004), lonely=4004)


# ---- the scenes of the colour tests (tests/test_color_reference.py, tests/test_gpu_color.py)
def frozen(a):
    a.setflags(write=False)
    return a


def texture(xy):
    """I = 0.5 + 0.2 sin(2 x) + 0.2 cos(1.7 y), rounded to float32"""
    return (0.5 + 0.2 * np.sin(2.0 * xy[:, 0]) + 0.2 * np.cos(1.7 * xy[:, 1])).astype(np.float32)


def scene(name):
    """"wave", "flat" or "shifted" -> dict(moving [3000, 3], ib [3000], fixed [4000, 3], normals [4000, 3], ia [4000], all float32, and the
    ground truth G as a float64 [4, 4]).  4 000 fixed points, x and y uniform in [-2, 2], on z = 0.3 sin(1.5 x) cos(1.2 y) ("wave";
    "shifted": the same moved by (100, -50, 25)) or on z = 0 exactly with normals (0, 0, 1) ("flat"); the moving cloud is 3 000 of
    them under the inverse of G: 5 degrees about (1, 2, 3) through the centroid plus (0.05, -0.03, 0.04), for "flat" 5 degrees about z
    plus (0.05, -0.03, 0).  Every moving point carries the intensity of the fixed point it was taken from."""
    rng = np.random.default_rng(97)
    xy = rng.uniform(-2, 2, (4000, 2))
    x, y = xy[:, 0], xy[:, 1]
    if name == "flat":
        fixed = np.stack([x, y, np.zeros(4000)], axis=1)
        normals = np.tile(np.array([0.0, 0.0, 1.0]), (4000, 1))
        axis, shift = np.array([0.0, 0.0, 1.0]), np.array([0.05, -0.03, 0.0])
    else:
        fixed = np.stack([x, y, 0.3 * np.sin(1.5 * x) * np.cos(1.2 * y)], axis=1)
        normals = np.stack([-0.45 * np.cos(1.5 * x) * np.cos(1.2 * y), 0.36 * np.sin(1.5 * x) * np.sin(1.2 * y), np.ones(4000)], axis=1)
        normals /= np.linalg.norm(normals, axis=1, keepdims=True)
        axis, shift = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0), np.array([0.05, -0.03, 0.04])
    ia = texture(xy)
    if name == "shifted":
        fixed = fixed + np.array([100.0, -50.0, 25.0])
    fixed = fixed.astype(np.float32)
    pick = rng.permutation(4000)[:3000]
    Rg = P.rodrigues(np.deg2rad(5.0) * axis)
    c = fixed.astype(np.float64).mean(axis=0)
    G = np.eye(4)
    G[:3, :3], G[:3, 3] = Rg, c + shift - Rg @ c
    moving = (fixed[pick].astype(np.float64) - G[:3, 3]) @ Rg                 # G^-1 p = Rg^T (p - t), row vectors
    if name == "flat":
        moving[:, 2] = 0.0                                                       # (a rotation about z: exactly in the plane)
    return dict(moving=frozen(moving.astype(np.float32)), ib=frozen(ia[pick].copy()), fixed=frozen(fixed), normals=frozen(normals.astype(np.float32)),
                ia=frozen(ia), G=frozen(G))
