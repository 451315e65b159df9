"""GPU suite of mi_knn_search, mi_estimate_normals and mi_remove_outliers at the grid shapes their own suites never plan: a clamped axis,
64 to 107 cells per axis, more queries than the radix sort's small path holds, and the radius grid at both bounds of its points-per-cell
rule.  The cases, the sampling of the O(n m) restatement and the size-independent checks: tests/search_scale_cases.py; that every case plans
the grid it is named for: tests/test_search_scale_regimes.py.

Nothing here has a tolerance of its own.  k-NN indices, distance bits and counts are compared bit for bit -- every row where the full
restatement is affordable (the clamped cloud), else every sampled row, and every row against the properties of its own answer.  Normals and
outlier scores go through the check functions of tests/test_gpu_normals.py and tests/test_gpu_outliers.py, with their bounds.

The restatement's FMA arithmetic costs about 1e-7 s per pair (float64 with its error term, knn_reference.fma_sq_f32), the other 2e-8 s: the
300 000-point clouds and the self-mode cloud of 4096 * 64 + 1 points are held against sampled rows in MI_DIST_CPU_ROUNDING alone; in
MI_DIST_FMA the 300 000-point clouds keep the per-row properties and, at k = 1, the grid 1-NN search's answer bit for bit."""
import numpy as np
import pytest

import knn_reference as K
import normals_reference as N
import outlier_reference as R
import search_scale_cases as S
from test_gpu_knn import check as knn_check
from test_gpu_normals import check as normals_check
from test_gpu_outliers import RADIUS, STATISTICAL, check_consistency, check_radius, check_statistical, fewer_outputs_agree, run

pytestmark = pytest.mark.gpu

MODES = S.MODES


def knn_call(ctx, query, cloud, k, mode):
    return ctx.knn_search(query, cloud, k, mode, want_d2=True, want_count=True)


def normals_call(ctx, cloud, k, mode):
    return ctx.estimate_normals(cloud, k, None, mode, want_curvature=True, want_count=True)


# ---- 1. a clamped axis: 1023 x 1 x 1 cells whose edge is the floor, queries up to 10 box lengths off either end
@pytest.mark.parametrize("self_mode", [False, True], ids=["queries", "self"])
@pytest.mark.parametrize("mode", MODES)
def test_clamped_axis_knn(ctx, capi, monkeypatch, mode, self_mode):
    cloud, query = S.clamped_cloud(), None if self_mode else S.clamped_queries()[0]
    keys = S.clamped_keys(mode, self_mode)                           # the full restatement: every row is compared
    for k in (8, 32):
        got = knn_check(ctx, query, cloud, k, mode, keys)
        S.check_knn_properties(got, query, cloud, k, mode, "clamped k %d mode %d" % (k, mode))
    # k = 32 at its default of 16 points per cell plans 376 cells: at one point per cell the floor holds for it too
    monkeypatch.setenv("MISLAM_KNN_POINTS_PER_CELL", "1")
    with capi.Context(0) as c2:
        knn_check(c2, query, cloud, 32, mode, keys)


@pytest.mark.parametrize("mode", MODES)
def test_clamped_axis_normals(ctx, mode):
    cloud = S.clamped_cloud()
    ref = N.from_neighbours(cloud, K.unpack(S.clamped_keys(mode, True), 8)[0])
    normals_check(ref, normals_call(ctx, cloud, 8, mode), "clamped normals mode %d" % mode, share=False)   # (a line has no eigen-gap)


@pytest.mark.parametrize("mode", MODES)
def test_clamped_axis_outliers(ctx, capi, mode):
    cloud = S.clamped_cloud()
    mu, count = R.scores(S.clamped_keys(mode, True), 8)
    for ratio in (0.0, 1.0, 2.0):
        got = run(ctx, capi, cloud, method=STATISTICAL, k=8, dist_mode=mode, std_ratio=ratio)
        check_statistical(cloud, got, mu, count, ratio, "clamped statistical mode %d ratio %g" % (mode, ratio))   # (no point within 1e-9 of the threshold)
    radius_count = R.radius_counts(cloud, S.CLAMPED_RADIUS, mode)
    assert radius_count.min() == 0 and radius_count.max() >= 32                  # from stray points to whole knots
    for min_nb in (1, 2, 40):
        fields = dict(method=RADIUS, radius=S.CLAMPED_RADIUS, min_neighbours=min_nb, dist_mode=mode)
        got = run(ctx, capi, cloud, **fields)
        check_radius(cloud, got, radius_count, min_nb, "clamped radius min %d mode %d" % (min_nb, mode))
        fewer_outputs_agree(ctx, capi, cloud, got, **fields)


# ---- 2. many cells per axis
def cells_check(c, capi, points, offset, mode, sampled):
    q, cloud = S.cells_case(points, offset)
    for k in S.CELLS_KS:
        what = "%d points + %g, k %d mode %d" % (points, offset, k, mode)
        got = knn_call(c, q, cloud, k, mode)
        S.check_knn_properties(got, q, cloud, k, mode, what)
        if sampled:
            rows, keys = S.cells_keys(points, offset, mode)
            S.check_knn_rows(got, rows, keys, k, what)
        if k == 1:
            nidx, nd2 = c.nn_search(q, cloud, mode, capi.NN_GRID)
            assert np.array_equal(got[0][:, 0], nidx) and np.array_equal(got[1][:, 0].view(np.uint32), nd2.view(np.uint32)), what


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("offset", [0.0, S.OFFSET])
def test_many_cells_per_axis(ctx, capi, offset, mode):
    """300 000 points: 67 cells per axis at k = 1 (43 and 33 at k = 8 and 17).  Sampled rows in MI_DIST_CPU_ROUNDING: see the head."""
    cells_check(ctx, capi, S.CELLS_POINTS, offset, mode, sampled=mode == K.DIST_CPU_ROUNDING)


@pytest.mark.parametrize("mode", MODES)
def test_many_cells_per_axis_at_a_quarter_point_per_cell(capi, monkeypatch, mode):
    """65 cells per axis over 66 000 points for every k, both arithmetics against sampled rows; and the 300 000 points at 107 per axis."""
    monkeypatch.setenv("MISLAM_KNN_POINTS_PER_CELL", S.FINE_PPC)
    with capi.Context(0) as c2:
        cells_check(c2, capi, S.FINE_POINTS, 0.0, mode, sampled=True)
        if mode == K.DIST_CPU_ROUNDING:
            cells_check(c2, capi, S.CELLS_POINTS, 0.0, mode, sampled=True)


# ---- 3. many queries: one more than 4096 * 64
@pytest.mark.parametrize("mode", MODES)
def test_many_queries(ctx, mode):
    q, cloud = S.many_queries_case()
    rows, keys = S.many_queries_keys(mode)
    what = "%d queries mode %d" % (len(q), mode)
    got = knn_call(ctx, q, cloud, S.MANY_K, mode)
    S.check_knn_rows(got, rows, keys, S.MANY_K, what)
    S.check_knn_properties(got, q, cloud, S.MANY_K, mode, what)


@pytest.fixture(scope="module")
def self_knn(ctx):
    """the device's k-NN answer on the self-mode cloud: compared in test_many_queries_self_mode, and what the whole-cloud restatements of
    the normals and the outlier scores below start from"""
    return knn_call(ctx, None, S.many_self_cloud(), S.MANY_K, S.MANY_SELF_MODE)


def test_many_queries_self_mode(self_knn):
    cloud = S.many_self_cloud()
    rows, keys = S.many_self_keys()
    S.check_knn_rows(self_knn, rows, keys, S.MANY_K, "self mode, %d points" % len(cloud))
    S.check_knn_properties(self_knn, None, cloud, S.MANY_K, S.MANY_SELF_MODE, "self mode, %d points" % len(cloud))


def test_many_queries_normals(ctx, self_knn):
    """Sampled rows against the restatement fed with the REFERENCE's neighbour rows; every row against the restatement fed with the
    device's own k-NN answer (which test_many_queries_self_mode holds to the reference)."""
    cloud = S.many_self_cloud()
    rows, keys = S.many_self_keys()
    got = normals_call(ctx, cloud, S.MANY_K, S.MANY_SELF_MODE)
    ref = S.normals_of_rows(cloud, rows, K.unpack(keys, S.MANY_K)[0])
    normals_check(ref, tuple(a[rows] for a in got), "normals, %d sampled rows" % len(rows))
    normals_check(N.from_neighbours(cloud, self_knn[0]), got, "normals, every row from the device's neighbours")


def test_many_queries_outliers(ctx, capi, self_knn):
    """mean_distance and neighbours of the sampled rows against the reference's scores, with the bound of test_gpu_outliers.py.

    The float64 reference of the global mean and standard deviation needs every row's neighbours, 6.9e10 pairs: not affordable, so the
    assertion against the REFERENCE's statistics is dropped.  In its place: the structural identities (check_consistency), and the whole of
    check_statistical -- statistics, mask and all -- against the restatement's scores computed from the device's own k-NN answer, which
    test_many_queries_self_mode holds to the reference on the sampled rows and to its own distances on every row."""
    cloud = S.many_self_cloud()
    rows, keys = S.many_self_keys()
    mu_rows, count_rows = R.scores(keys, S.MANY_K)
    mu, count = R.scores(S.device_keys(self_knn[0], self_knn[1]), S.MANY_K)
    assert np.array_equal(mu[rows], mu_rows) and np.array_equal(count[rows], count_rows)
    for ratio in (0.0, 2.0):
        got = run(ctx, capi, cloud, method=STATISTICAL, k=S.MANY_K, dist_mode=S.MANY_SELF_MODE, std_ratio=ratio)
        md = got["mean_distance"][rows].astype(np.float64)
        assert np.array_equal(got["neighbours"][rows], count_rows)
        assert (np.abs(md - mu_rows) <= 6e-8 * mu_rows).all() and (md[mu_rows == 0] == 0).all()      # check_statistical's comparison, on the sample
        check_consistency(cloud, got, "statistical, %d points" % len(cloud))
        assert got["stats"][3] == int(got["keep"].sum()) and np.array_equal(got["index"], np.flatnonzero(got["keep"]))
        assert (np.diff(got["index"]) > 0).all()
        check_statistical(cloud, got, mu, count, ratio, "statistical, every row from the device's neighbours, ratio %g" % ratio, cap=False)


# ---- 4. the radius grid at both bounds of its rule: a 41^3 lattice, every point alone / one spacing / everything a neighbour
@pytest.fixture(scope="module")
def lattice_reference():
    """{radius: (sampled rows, outlier_reference's counts of them)}.  Every squared distance of the lattice is an integer below 2^13, exact
    in both arithmetics -- held on 64 of the rows -- so one restatement serves both; the geometry's counts for EVERY point (S.lattice_counts)
    are held against it on the sampled rows."""
    L = S.lattice()
    rows = S.sample_rows(len(L), 512, 139)
    out = {}
    for radius in S.RADII:
        count = R.radius_counts(L, radius, K.DIST_CPU_ROUNDING, block=S.reference_block(len(L)), only=rows)
        assert np.array_equal(R.radius_counts(L, radius, K.DIST_FMA, block=S.reference_block(len(L)), only=rows[::8]), count[::8])
        assert np.array_equal(S.lattice_counts(radius)[rows], count)
        out[radius] = (rows, count)
    return out


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("radius", S.RADII)
def test_radius_grid_bounds(ctx, capi, lattice_reference, radius, mode):
    L = S.lattice()
    rows, count_rows = lattice_reference[radius]
    count = S.lattice_counts(radius)
    most = int(count.max())                                           # 0, 6, n - 1: thresholds at it, one below and one above (all >= 1)
    for min_nb in sorted({max(most - 1, 1), max(most, 1), max(most, 1) + 1}):
        what = "lattice radius %g min %d mode %d" % (radius, min_nb, mode)
        fields = dict(method=RADIUS, radius=radius, min_neighbours=min_nb, dist_mode=mode)
        got = run(ctx, capi, L, **fields)
        assert np.array_equal(got["neighbours"][rows], count_rows), what                             # outlier_reference, the sampled rows
        assert np.array_equal(got["keep"][rows].astype(bool), count_rows >= min_nb), what
        check_radius(L, got, count, min_nb, what)                                                    # every row
        fewer_outputs_agree(ctx, capi, L, got, **fields)                                             # (without neighbours: the early-exit kernel)
