"""The problems the batched-ICP suites run, generated from seeds: no fixture files.

A problem is a pair (moving cloud, fixed cloud).  The well-posed ones are two independent samples of one smooth seeded surface, the
moving one displaced by a random rigid motion and perturbed by noise -- small enough motions that the every-pair correspondences pull
the clouds together, large enough that a registration takes tens of iterations.  The ill-posed ones are the rank-deficient solves the
single call's suite uses for the out-of-line IEEE path."""
import numpy as np

SIZES = (1, 2, 3, 63, 64, 65, 127, 128, 129, 1000, 2047, 2048, 4095, 4096)


def rotation(rng, max_angle):
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    ang = rng.uniform(0.3, 1.0) * max_angle
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * (K @ K)


def surface(rng, n, coeff, extent=1.0):
    """n points of the height field z = sum_k c_k sin(a_k x + p_k) cos(b_k y + q_k) over [-extent, extent]^2."""
    xy = rng.uniform(-extent, extent, (n, 2))
    z = np.zeros(n)
    for c, a, b, p, q in coeff:
        z += c * np.sin(a * xy[:, 0] + p) * np.cos(b * xy[:, 1] + q)
    return np.column_stack([xy, z])


def pair(seed, n, m, max_angle=0.25, max_shift=0.15, noise=0.002, extent=1.0):
    rng = np.random.default_rng(seed)
    coeff = [(rng.uniform(0.1, 0.3), rng.uniform(1, 4), rng.uniform(1, 4), rng.uniform(0, 6), rng.uniform(0, 6)) for _ in range(3)]
    fixed = surface(rng, m, coeff, extent)
    moving = surface(rng, n, coeff, extent)
    R = rotation(rng, max_angle)
    t = rng.uniform(-max_shift, max_shift, 3)
    moving = (moving - t) @ R + rng.normal(0, noise, (n, 3))      # R^T (p - t): the registration has to find (R, t)
    return moving.astype(np.float32), fixed.astype(np.float32)


def sizes_batch(seed=1000):
    """All 196 moving x fixed size combinations of SIZES."""
    out = []
    for i, n in enumerate(SIZES):
        for j, m in enumerate(SIZES):
            out.append(pair(seed + 20 * i + j, n, m))
    return out


def rules_batch(seed=5000, count=40):
    """40 problems of mixed sizes between 1000 and 3000 points that CONVERGE under the default eps = 1e-3: over [-0.5, 0.5]^2 a fixed cloud
    of m >= 1000 points leaves an aligned moving point a mean squared distance of ~ 1 / (pi m) <= 3.2e-4 to its nearest neighbour, below
    eps.  (A cloud too sparse for eps runs to the iteration cap, where one flipped near-tie correspondence separates any two correct fp32
    implementations: such a run says nothing about either.)"""
    rng = np.random.default_rng(seed)
    return [pair(seed + 1 + k, int(rng.integers(1000, 3000)), int(rng.integers(1000, 3000)), extent=0.5) for k in range(count)]


def small_batch(seed=9000, count=1500, lo=1, hi=512):
    rng = np.random.default_rng(seed)
    return [pair(seed + 1 + k, int(rng.integers(lo, hi + 1)), int(rng.integers(lo, hi + 1))) for k in range(count)]


def ill_posed(seed=7000):
    """(name, moving, fixed): planar, collinear, all points equal, a lattice against itself shifted by half a cell (distance ties), offset 1e3."""
    rng = np.random.default_rng(seed)
    out = []
    plane = np.column_stack([rng.uniform(-1, 1, (1500, 2)), np.zeros(1500)])
    Rm = rotation(rng, 0.2)
    out.append(("planar", plane @ Rm.T + 0.05, plane[rng.permutation(1500)[:1200]]))
    line = np.outer(rng.uniform(-1, 1, 700), np.array([1.0, 2.0, -0.5]))
    out.append(("collinear", line @ Rm.T + 0.02, line[:650]))
    out.append(("collinear_moving_only", line @ Rm.T + 0.02, pair(seed + 1, 10, 900)[1]))
    out.append(("all_equal", np.tile(np.array([[0.25, -0.5, 0.75]]), (300, 1)), pair(seed + 2, 10, 500)[1]))
    out.append(("all_equal_both", np.tile(np.array([[0.25, -0.5, 0.75]]), (300, 1)), np.tile(np.array([[0.5, 0.5, 0.5]]), (200, 1))))
    g = np.arange(12, dtype=np.float64)
    lattice = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3) * 0.125
    out.append(("lattice_half_cell", lattice + 0.0625, lattice))
    out.append(("lattice_half_cell_x", lattice + np.array([0.0625, 0, 0]), lattice))
    b, a = pair(seed + 3, 1800, 2100)
    out.append(("offset_1e3", b + 1000.0, a + 1000.0))
    dup = pair(seed + 4, 600, 800)
    out.append(("duplicates", np.concatenate([dup[0], dup[0]]), np.concatenate([dup[1], dup[1][:300]])))
    return [(name, np.ascontiguousarray(b, np.float32), np.ascontiguousarray(a, np.float32)) for name, b, a in out]


def stop_reason_problems(seed=8000):
    """Problems aimed at each stop reason: (name, moving, fixed, params keywords).  The suite checks with the single call that each reason is hit."""
    b, a = pair(seed, 900, 1100)
    out = [("converged", a[:800].copy(), a, dict()),                                         # identical points: error 0 in the first check
           ("max_iterations", b, a, dict(max_iterations=3)),
           ("no_pairs", b + np.float32(50.0), a, dict(filter_pairs=1, max_distance_squared=1.0))]     # the gap is ~50 units
    for k in range(12):                                                                       # cuda-slam's rules: abort when the error rises
        bb, aa = pair(seed + 10 + k, 300 + 40 * k, 250 + 30 * k, max_angle=0.6, max_shift=0.3, noise=0.01)
        out.append(("abort_%d" % k, bb, aa, dict(cuda_slam=True, eps=1e-7, max_iterations=200)))
    return out
