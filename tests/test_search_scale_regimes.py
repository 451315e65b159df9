"""Every case of tests/test_gpu_search_scale.py reaches the grid shape it is named for -- by the numpy restatement of the plan in
tests/search_scale_cases.py (grid_plan of csrc/nn_grid.hip, knn_default_points_per_cell, radius_points_per_cell), no device needed.  If the
plan's constants change, this says which case no longer tests what it claims."""
import numpy as np

import search_scale_cases as S


def test_the_restated_plan_on_grids_known_by_hand():
    rng = np.random.default_rng(5)
    c = rng.uniform(0, 1, (1000, 3)).astype(np.float32)
    c[0], c[1] = 0.0, 1.0
    dims, inv_h, raised = S.grid_plan(c, 1.0)                       # 1000 cells of edge 0.1; the upper face's points open an 11th layer
    assert dims.tolist() == [11, 11, 11] and abs(float(inv_h) - 10.0) < 1e-5 and not raised
    dims, inv_h, raised = S.grid_plan(c, 1e9)                       # one cell's worth of points: edge 1, and again the upper face
    assert dims.tolist() == [2, 2, 2] and inv_h == 1.0 and not raised
    flat = c.copy()
    flat[:, 2] = 0.5                                                # a flat axis is one layer; its cells are spent on the other two
    dims, inv_h, raised = S.grid_plan(flat, 1.0)
    assert dims.tolist() == [32, 32, 1] and not raised
    assert S.knn_default_points_per_cell(1) == 1.0 and S.knn_default_points_per_cell(8) == 4.0 and S.knn_default_points_per_cell(17) == 8.5


def test_cases_reach_the_regimes_they_are_named_for():
    # ---- a clamped axis: >= 1000 cells on x, and the cell edge is the floor ext_max / (GRID_MAX_DIM - 2), not what the points ask for
    cloud = S.clamped_cloud()
    queries, groups = S.clamped_queries()
    assert cloud.shape == (S.CLAMPED_POINTS, 3) and queries.shape == (512, 3) and sum(len(g) for g in groups.values()) == 512
    lo, hi = cloud.min(axis=0), cloud.max(axis=0)
    assert lo[0] == 0 and hi[0] == np.float32(S.CLAMPED_LENGTH) and lo[1] == hi[1] == 0 and 0 < hi[2] - lo[2] < 1e-2
    radius_ppc, bound = S.radius_points_per_cell(cloud, S.CLAMPED_RADIUS)
    clamped_plans = {"k 8 (k-NN, normals, statistical outliers)": S.knn_default_points_per_cell(8),
                     "MISLAM_KNN_POINTS_PER_CELL = 1 (the k 32 run)": 1.0, "radius outliers": radius_ppc}
    for what, ppc in clamped_plans.items():
        dims, inv_h, raised = S.grid_plan(cloud, ppc)
        assert raised and dims[0] >= 1000 and dims[0] <= S.GRID_MAX_DIM and dims[1] == dims[2] == 1, (what, dims)
    assert not S.grid_plan(cloud, S.knn_default_points_per_cell(32))[2]        # (k 32 at its default asks for 375 cells: hence the run above)
    inside = (queries >= lo).all(axis=1) & (queries <= hi).all(axis=1)
    assert inside[groups["line"]].all() and inside[groups["faces"]].all()
    assert ((queries[groups["faces"]] == lo) | (queries[groups["faces"]] == hi)).any(axis=1).all()
    assert not inside[groups["near"]].any() and not inside[groups["beyond"]].any() and not inside[groups["off_axis"]].any()
    ends = S.cell_of(cloud, 4.0, queries[groups["beyond"]])[:, 0]
    nx = S.grid_plan(cloud, 4.0)[0][0]
    assert set(ends.tolist()) == {0, nx - 1}                                   # both ends, each clamped into the grid's last cell
    assert np.abs(queries[groups["beyond"], 0] - 5e5).min() >= 10 * S.CLAMPED_LENGTH
    assert np.abs(queries[groups["off_axis"], 1:]).max(axis=1).min() >= 500

    # ---- many cells per axis: >= 64 on every axis
    for offset in (0.0, S.OFFSET):
        q, c = S.cells_case(S.CELLS_POINTS, offset)
        assert q.shape == (S.CELLS_QUERIES, 3) and c.shape == (S.CELLS_POINTS, 3)
        dims, _, raised = S.grid_plan(c, S.knn_default_points_per_cell(1))
        assert (dims >= 64).all() and not raised, dims                        # k 1 at its default; k 8 and 17 plan 43 and 33 cells per axis ...
        dims, _, raised = S.grid_plan(c, float(S.FINE_PPC))
        assert (dims >= 64).all() and (dims <= 200).all() and not raised, dims    # ... and reach 107 at 0.25 points per cell: a table of 1.2e6 cells
        out = ((q < c.min(axis=0)) | (q > c.max(axis=0))).any(axis=1)
        on_face = ((q == c.min(axis=0)) | (q == c.max(axis=0))).any(axis=1)
        assert out.sum() >= 400 and on_face.sum() >= 400 and (~out & ~on_face).sum() >= 900
    q, c = S.cells_case(S.FINE_POINTS, 0.0)
    dims, _, raised = S.grid_plan(c, float(S.FINE_PPC))
    assert (dims >= 64).all() and not raised, dims
    assert (S.grid_plan(c[:60_000], float(S.FINE_PPC))[0] < 64).all()          # (60 000 points would stop at 63)

    # ---- many queries: one more than the radix sort's small path holds; the self-mode cloud is as large
    assert S.MANY == S.SORT_ONE_PASS + 1
    assert S.many_queries_case()[0].shape == (S.MANY, 3) and S.many_self_cloud().shape == (S.MANY, 3)
    for rows in (S.sample_rows(S.MANY, 512, 1), S.sample_rows(S.MANY, 1024, 2)):
        assert {0, S.SORT_ONE_PASS - 1, S.SORT_ONE_PASS, S.MANY - 1} <= set(rows.tolist()) and len(set(rows.tolist())) == len(rows) >= 512

    # ---- the radius grid at both bounds of radius_points_per_cell
    L = S.lattice()
    n = len(L)
    assert n == S.LATTICE_SIDE ** 3 and (L.max(axis=0) - L.min(axis=0) == 40).all()
    ppc, bound = S.radius_points_per_cell(L, S.RADII[0])
    dims, _, _ = S.grid_plan(L, ppc)
    assert bound == "floor" and ppc == 1.0 and np.prod(dims) >= n                # at most one point per cell asked for: every point alone
    ppc, bound = S.radius_points_per_cell(L, S.RADII[1])
    dims, inv_h, _ = S.grid_plan(L, ppc)
    assert bound == "between" and inv_h == 1.0 and dims.tolist() == [41, 41, 41]  # cells of one lattice spacing: every face on the lattice
    ppc, bound = S.radius_points_per_cell(L, S.RADII[2])
    dims, inv_h, _ = S.grid_plan(L, ppc)
    # one cell asked for, its edge the box's: grid_plan opens a second layer per axis for the points ON the upper faces (u = 1 exactly)
    assert bound == "one cell" and ppc == n and np.float32(40) * inv_h == 1.0 and dims.tolist() == [2, 2, 2]
    for radius in S.RADII:
        assert S.lattice_counts(radius).shape == (n,)
