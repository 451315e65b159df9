"""The cases of tests/test_gpu_search_scale.py and what they share: the clouds and queries that take mi_knn_search, mi_estimate_normals and
mi_remove_outliers to the grid shapes the small suites never plan (a clamped axis, 64 and more cells per axis, more queries than the radix
sort's one-workgroup path holds, the radius grid at both bounds of its points-per-cell rule), a numpy restatement of the plan's arithmetic
(grid_plan of csrc/nn_grid.hip, dimensions and inv_h only; the points-per-cell rules of csrc/search_front.hip and csrc/outlier_api.hip) that
tests/test_search_scale_regimes.py holds every case against, and the checks of a device answer that do not grow with the case:

  sampled rows   a fixed, seeded sample of rows against the restatement of tests/knn_reference.py, bit for bit -- always with the first
                 row, the last one and the two rows either side of index 4096 * 64 where the case has them
  every row      properties stated on the device's own answer: the d2 bits are the distance to the reported index in the call's
                 arithmetic (the expression of knn_reference.d2_matrix, per pair); keys ascend strictly; no index twice; count = the
                 finite slots; in self mode row i never holds i

No tolerance is introduced here: the k-NN answer is compared bit for bit, the normals and the outlier scores go through the `check`
functions of tests/test_gpu_normals.py and tests/test_gpu_outliers.py with their bounds."""
import functools

import numpy as np

import knn_reference as K
import normals_reference as N

MODES = (K.DIST_CPU_ROUNDING, K.DIST_FMA)
SORT_ONE_PASS = 4096 * 64            # keys up to which the library's radix sort (morton_order runs on it) takes its small path: tests/test_gpu_sort.py
GRID_MAX_DIM = 1024                  # csrc/nn_grid.h


def frozen(a):
    a.setflags(write=False)
    return a


# ---- the plan, restated (dimensions and inv_h only)
def knn_default_points_per_cell(k):
    return max(1.0, 0.5 * k)


def radius_points_per_cell(cloud, radius, cell_in_radii=1.0):
    """radius_points_per_cell of csrc/outlier_api.hip -> (ppc, "floor" / "one cell" / "between")"""
    lo, hi = cloud.min(axis=0).astype(np.float64), cloud.max(axis=0).astype(np.float64)
    edge = float(cell_in_radii) * float(np.float32(radius))
    cells = 1.0
    for ext in hi - lo:
        if ext > edge:
            cells *= ext / edge
    n = len(cloud)
    ppc = n / cells
    bound = "floor" if ppc <= knn_default_points_per_cell(1) else ("one cell" if cells == 1.0 else "between")
    return float(np.float32(min(max(ppc, knn_default_points_per_cell(1)), float(n)))), bound


def grid_plan(cloud, points_per_cell):
    """grid_plan of csrc/nn_grid.hip for the grid over `cloud` -> (dims int [3], inv_h float32, whether h was raised to the floor
    ext_max / (GRID_MAX_DIM - 2))."""
    lo, hi = cloud.min(axis=0), cloud.max(axis=0)                    # float32, as the range pass gives them
    ext = hi.astype(np.float64) - lo.astype(np.float64)
    active = (ext > 0) & np.isfinite(ext)
    cells = max(1.0, len(cloud) / float(np.float32(points_per_cell)))
    h = 1.0
    for _ in range(4):
        d = int(active.sum())
        if d == 0:
            h = 1.0
            break
        h = float(np.prod(ext[active]) / cells) ** (1.0 / d)
        flat = active & (ext < h)                                    # a flat axis: one layer of cells
        if not flat.any():
            break
        active &= ~flat
    floor = float(ext.max()) / (GRID_MAX_DIM - 2)
    raised = bool(ext.max() > 0 and floor > h)
    if raised:
        h = floor
    inv_h = np.float32(1.0 / h)
    for _ in range(8):
        umax = (hi - lo) * inv_h                                     # float32: cell_u of the box's upper corner
        dims = np.where(np.isfinite(umax) & (umax > 0), np.floor(umax) + 1, 1).astype(np.int64)
        if (dims <= GRID_MAX_DIM).all():
            break
        inv_h = inv_h * np.float32(0.5)
    return np.clip(dims, 1, GRID_MAX_DIM), inv_h, raised


def cell_of(cloud, points_per_cell, points):
    """the (clamped) cell of every point of `points` in the grid planned over `cloud`: int [n, 3]"""
    dims, inv_h, _ = grid_plan(cloud, points_per_cell)
    u = (np.ascontiguousarray(points, np.float32) - cloud.min(axis=0)) * inv_h
    return np.minimum(np.maximum(np.floor(u), 0), (dims - 1).astype(np.float32)).astype(np.int64)


# ---- 1. a clamped axis
CLAMPED_POINTS, CLAMPED_LENGTH, CLAMPED_KNOTS = 6000, 1e6, 40
CLAMPED_RADIUS = 300.0               # about the spacing of the cloud's uniform half: neighbour counts from 0 to a knot's size


@functools.lru_cache(maxsize=None)
def clamped_cloud():
    """6 000 points along x over [0, 1e6]: half uniform, half in 40 knots of sigma 0.01 (far below fp32's spacing up there: stacks of equal
    x); y = 0, z ~ N(0, 1e-4).  The x axis alone asks for thousands of cells."""
    rng = np.random.default_rng(101)
    half = CLAMPED_POINTS // 2
    x = rng.uniform(0, CLAMPED_LENGTH, half)
    x[0], x[1] = 0.0, CLAMPED_LENGTH                                  # the box is the stated one
    centre = rng.uniform(0, CLAMPED_LENGTH, CLAMPED_KNOTS)
    knots = np.clip(centre[rng.integers(0, CLAMPED_KNOTS, half)] + rng.normal(0, 0.01, half), 0, CLAMPED_LENGTH)
    x = np.concatenate([x, knots])[rng.permutation(CLAMPED_POINTS)]
    return frozen(np.stack([x, np.zeros(CLAMPED_POINTS), rng.normal(0, 1e-4, CLAMPED_POINTS)], axis=1).astype(np.float32))


CLAMPED_GROUPS = ("line", "faces", "near", "beyond", "off_axis")


@functools.lru_cache(maxsize=None)
def clamped_queries():
    """512 queries -> (float32 [512, 3], {group: rows}): on the line, on the bounding box's faces, 1e-3 outside it (one fp32 step where 1e-3
    is below the spacing), 10 box lengths beyond either end, and far off the axis."""
    rng = np.random.default_rng(103)
    cloud = clamped_cloud()
    lo, hi = cloud.min(axis=0).astype(np.float64), cloud.max(axis=0).astype(np.float64)

    def inside(n):
        return rng.uniform(lo, hi, (n, 3))

    line = inside(103)
    line[:, 2] = 0
    faces, near = inside(103), inside(102)
    axis, side = rng.integers(0, 3, 103), rng.integers(0, 2, 103)
    faces[np.arange(103), axis] = np.where(side == 0, lo[axis], hi[axis])
    axis, side = rng.integers(0, 3, 102), rng.integers(0, 2, 102)
    near[np.arange(102), axis] = np.where(side == 0, lo[axis] - 1e-3, hi[axis] + 1e-3)
    beyond = inside(102)
    beyond[:, 0] = np.where(rng.integers(0, 2, 102) == 0, lo[0] - 10 * CLAMPED_LENGTH, hi[0] + 10 * CLAMPED_LENGTH)
    beyond[:, 1:] += rng.normal(0, 1.0, (102, 2))
    off = inside(102)
    off[:, 1:] += rng.choice([-1.0, 1.0], (102, 2)) * rng.choice([1e3, 1e6, 1e7], (102, 1)) * rng.uniform(0.5, 1, (102, 2))
    q = np.concatenate([line, faces, near, beyond, off]).astype(np.float32)
    # 1e-3 beyond x = 1e6 rounds back onto the face (the spacing there is 0.0625): the next float instead
    q[206 + np.flatnonzero((axis == 0) & (side == 1)), 0] = np.nextafter(np.float32(hi[0]), np.float32(np.inf))
    bounds = np.cumsum([0, 103, 103, 102, 102, 102])
    return frozen(q), {name: np.arange(bounds[i], bounds[i + 1]) for i, name in enumerate(CLAMPED_GROUPS)}


@functools.lru_cache(maxsize=None)
def clamped_keys(mode, self_mode):
    return frozen(K.sorted_keys(None if self_mode else clamped_queries()[0], clamped_cloud(), mode))


# ---- 2. many cells per axis
CELLS_POINTS, CELLS_QUERIES, CELLS_KS = 300_000, 2000, (1, 8, 17)
# 0.25 points per cell: 65 cells per axis need 64^3 * 0.25 = 65 536 points and a little room
FINE_POINTS, FINE_PPC = 66_000, "0.25"
OFFSET = 1e3                          # fp32 spacing 6.1e-5 at 1e3 against a point spacing of 0.15: exact ties between distances begin


def box_queries(rng, lo, hi, n):
    """n queries around the box [lo, hi]: half inside, a quarter on its faces, a quarter outside (1e-3, then up to a box length away)"""
    q = rng.uniform(lo, hi, (n, 3))
    rest = np.arange(n // 2, n)
    axis, side = rng.integers(0, 3, len(rest)), rng.integers(0, 2, len(rest))
    out = np.zeros(len(rest))
    third = len(rest) // 2
    out[third:third + third // 2] = 1e-3
    out[third + third // 2:] = rng.uniform(0, 1, len(rest) - third - third // 2) * (hi - lo).max()
    q[rest, axis] = np.where(side == 0, lo[axis] - out, hi[axis] + out)
    return q


@functools.lru_cache(maxsize=None)
def cells_case(points, offset):
    """(queries float32 [2000, 3], cloud float32 [points, 3]): a uniform cloud in [-5, 5]^3 (+ offset), queries inside, on the faces, outside"""
    rng = np.random.default_rng(107 + points)
    cloud = (rng.uniform(-5, 5, (points, 3)) + offset).astype(np.float32)
    lo, hi = cloud.min(axis=0).astype(np.float64), cloud.max(axis=0).astype(np.float64)
    return frozen(box_queries(rng, lo, hi, CELLS_QUERIES).astype(np.float32)), frozen(cloud)


@functools.lru_cache(maxsize=None)
def cells_keys(points, offset, mode):
    """-> (the sampled query rows, their sorted keys)"""
    q, c = cells_case(points, offset)
    rows = sample_rows(len(q), 512, 109)
    return frozen(rows), frozen(K.sorted_keys(q, c, mode, block=reference_block(len(c)), only=rows))


# ---- 3. many queries
MANY = SORT_ONE_PASS + 1
MANY_CLOUD, MANY_K = 2000, 8


@functools.lru_cache(maxsize=None)
def many_queries_case():
    rng = np.random.default_rng(113)
    cloud = rng.uniform(-5, 5, (MANY_CLOUD, 3)).astype(np.float32)
    return frozen(box_queries(rng, np.full(3, -5.0), np.full(3, 5.0), MANY).astype(np.float32)), frozen(cloud)


@functools.lru_cache(maxsize=None)
def many_queries_keys(mode):
    q, c = many_queries_case()
    rows = sample_rows(MANY, 1024, 127)
    return frozen(rows), frozen(K.sorted_keys(q, c, mode, only=rows))


MANY_SELF_MODE = K.DIST_CPU_ROUNDING      # (the restatement's other arithmetic costs 1e-7 s per pair: 512 rows of this cloud would take 13 s)


@functools.lru_cache(maxsize=None)
def many_self_cloud():
    return frozen(np.random.default_rng(131).uniform(-5, 5, (MANY, 3)).astype(np.float32))


@functools.lru_cache(maxsize=None)
def many_self_keys():
    """-> (the sampled rows, their self-mode sorted keys): shared by the k-NN, the normals and the outlier test of the cloud"""
    c = many_self_cloud()
    rows = sample_rows(MANY, 512, 137)
    return frozen(rows), frozen(K.sorted_keys(None, c, MANY_SELF_MODE, block=reference_block(MANY), only=rows))


# ---- 4. the radius grid at both bounds of its rule
LATTICE_SIDE = 41
RADII = (1e-3, 1.0, 1e4)              # every point alone; one lattice spacing; everything a neighbour


@functools.lru_cache(maxsize=None)
def lattice():
    g = np.arange(LATTICE_SIDE, dtype=np.float32)
    z, y, x = np.meshgrid(g, g, g, indexing="ij")
    return frozen(np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1))      # index = x + side y + side^2 z; the box is 40 units


def lattice_counts(radius):
    """what the lattice's geometry gives (every squared distance is a small integer, exact in both arithmetics): int32 [n]"""
    L = lattice()
    if radius == RADII[0]:
        return np.zeros(len(L), np.int32)
    if radius == RADII[1]:
        return (6 - ((L == 0) | (L == LATTICE_SIDE - 1)).sum(axis=1)).astype(np.int32)
    assert radius == RADII[2]
    return np.full(len(L), len(L) - 1, np.int32)


# ---- the checks
def reference_block(m):
    """rows of the restatement worked at a time against a cloud of m points: about 4M pairs, whatever m"""
    return max(1, min(256, (1 << 22) // m))


def sample_rows(n, count, seed):
    """`count` rows of n, ascending: a seeded draw, with row 0, row n - 1 and the rows either side of index SORT_ONE_PASS always in"""
    forced = [r for r in (0, n - 1, SORT_ONE_PASS - 1, SORT_ONE_PASS) if 0 <= r < n]
    if count >= n:
        return np.arange(n)
    drawn = np.random.default_rng(seed).choice(n, count, replace=False)
    rows = np.unique(np.concatenate([drawn, forced]))
    assert set(forced) <= set(rows.tolist())
    return rows


def pair_d2(query, cloud, idx, mode):
    """float32 [n, k]: |cloud[idx[i, s]] - query[i]|^2 in the arithmetic of `mode` -- the expression of knn_reference.d2_matrix per pair
    (slots without a neighbour, idx -1, are computed against point 0 and to be ignored)"""
    c = cloud[np.where(idx >= 0, idx, 0)]
    dx, dy, dz = (c[:, :, a] - query[:, None, a] for a in range(3))
    if mode == K.DIST_CPU_ROUNDING:
        return (dx * dx + dy * dy) + dz * dz
    assert mode == K.DIST_FMA
    return K.fma_sq_f32(dz, K.fma_sq_f32(dy, dx * dx))


def check_knn_rows(got, rows, keys, k, what):
    """the rows `rows` of a device answer (idx, d2, count) against their sorted keys: every one of them, bit for bit"""
    want = K.unpack(keys, k)
    idx, d2, count = got[0][rows], got[1][rows], got[2][rows]
    bad = np.flatnonzero((idx != want[0]).any(axis=1) | (d2.view(np.uint32) != want[1].view(np.uint32)).any(axis=1) | (count != want[2]))
    assert bad.size == 0, "%s k %d: %d of %d sampled rows differ, first row %d: got %s %s (%d), want %s %s (%d)" % (
        what, k, bad.size, len(rows), rows[bad[0]], idx[bad[0]], d2[bad[0]], count[bad[0]], want[0][bad[0]], want[1][bad[0]], want[2][bad[0]])


def check_knn_properties(got, query, cloud, k, mode, what):
    """every row of a device answer (idx, d2, count) against itself; query None: self mode"""
    idx, d2, count = got
    self_mode = query is None
    query = cloud if self_mode else query
    n, m = len(query), len(cloud)
    assert idx.shape == d2.shape == (n, k) and count.shape == (n,), what
    have = idx >= 0
    assert ((idx >= -1) & (idx < m)).all(), what
    assert np.array_equal(np.isposinf(d2), ~have) and not np.isnan(d2).any(), what                   # a slot is filled or (-1, +inf)
    assert np.array_equal(count, have.sum(axis=1)), what
    assert (count == min(k, m - 1 if self_mode else m)).all(), what                                 # (no distance limit in these calls)
    wrong = have & (pair_d2(query, cloud, idx, mode).view(np.uint32) != d2.view(np.uint32))
    assert not wrong.any(), "%s: %d slots whose d2 is not the distance to their index, first in row %d" % (what, wrong.sum(), np.flatnonzero(wrong.any(axis=1))[0])
    keys = (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | idx.view(np.uint32).astype(np.uint64)
    rising = (keys[:, 1:] > keys[:, :-1]) | (keys[:, 1:] == K.KEY_EMPTY)
    assert rising.all(), "%s: keys do not ascend in row %d" % (what, np.flatnonzero(~rising.all(axis=1))[0])
    ordered = np.sort(idx, axis=1)
    twice = (ordered[:, 1:] == ordered[:, :-1]) & (ordered[:, 1:] >= 0)
    assert not twice.any(), "%s: an index twice in row %d" % (what, np.flatnonzero(twice.any(axis=1))[0])
    if self_mode:
        own = idx == np.arange(n)[:, None]
        assert not own.any(), "%s: row %d holds itself" % (what, np.flatnonzero(own.any(axis=1))[0])


def device_keys(idx, d2):
    """a device answer as sorted keys, for the restatements that start from them (outlier_reference.scores)"""
    return (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | idx.view(np.uint32).astype(np.uint64)


def normals_of_rows(cloud, rows, neighbours):
    """normals_reference.from_neighbours for the points `rows` alone, given their neighbour rows [len(rows), k]: the points and their
    neighbours are laid out as a small cloud of their own (the rows first), which is all the restatement reads."""
    s, k = neighbours.shape
    have = neighbours >= 0
    small = np.concatenate([cloud[rows], cloud[np.where(have, neighbours, 0)].reshape(s * k, 3)])
    idx = np.full((len(small), k), -1, np.int64)
    idx[:s] = np.where(have, s + np.arange(s * k).reshape(s, k), -1)
    lam, normal, C, count = N.from_neighbours(small, idx)
    return lam[:s], normal[:s], C[:s], count[:s]
