"""GPU suite of mi_knn_search: indices, distance bits and counts against the restatement of tests/knn_reference.py, bit for bit --
no tolerance anywhere.  The reference's sorted keys are built once per cloud pair and arithmetic (lru_cache) and shared by every k."""
import functools

import numpy as np
import pytest

import knn_reference as K

pytestmark = pytest.mark.gpu

MODES = (K.DIST_CPU_ROUNDING, K.DIST_FMA)
CELL_REGIMES = ("0.25", "1", "8", "64", "1e9")      # MISLAM_KNN_POINTS_PER_CELL: many shells ... one cell


def frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def uniform_pair(n, m, scale, seed=17):
    rng = np.random.default_rng(seed + 1000 * n + m)
    q = (rng.uniform(-5, 5, (n, 3)) * scale).astype(np.float32)
    c = (rng.uniform(-5, 5, (m, 3)) * scale).astype(np.float32)
    return frozen(q), frozen(c)


@functools.lru_cache(maxsize=None)
def uniform_keys(n, m, scale, mode):
    q, c = uniform_pair(n, m, scale)
    return frozen(K.sorted_keys(q, c, mode))


def same_bits(got, want):
    return all(np.array_equal(np.ascontiguousarray(g).view(np.uint32), np.ascontiguousarray(w).view(np.uint32)) for g, w in zip(got, want))


def check(ctx, query, cloud, k, mode, keys=None, max_d2=np.inf):
    """One device call against the restatement: idx, d2 bits and count."""
    if keys is None:
        keys = K.sorted_keys(query, cloud, mode, max_d2)
    want = K.unpack(keys, k)
    got = ctx.knn_search(query, cloud, k, mode, max_d2, want_d2=True, want_count=True)
    bad = np.flatnonzero((got[0] != want[0]).any(axis=1) | (got[1].view(np.uint32) != want[1].view(np.uint32)).any(axis=1) | (got[2] != want[2]))
    assert bad.size == 0, "k %d mode %d: %d rows differ, first %d: got %s %s (%d), want %s %s (%d)" % (
        k, mode, bad.size, bad[0], got[0][bad[0]], got[1][bad[0]], got[2][bad[0]], want[0][bad[0]], want[1][bad[0]], want[2][bad[0]])
    return got


# ---- 1. random clouds, both arithmetics, every list size at its edge and one past it
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("scale", [1.0, 100.0])
@pytest.mark.parametrize("k", [1, 2, 8, 9, 16, 17, 32])
@pytest.mark.parametrize("n,m", [(1, 1), (1, 17), (63, 5), (64, 64), (65, 1000), (1000, 333), (1000, 5000)])
def test_random_clouds(ctx, capi, n, m, k, scale, mode):
    q, c = uniform_pair(n, m, scale)
    idx, d2, count = check(ctx, q, c, k, mode, uniform_keys(n, m, scale, mode))
    if k == 1:
        for nn_mode in (capi.NN_BRUTEFORCE, capi.NN_TREE, capi.NN_GRID):
            nidx, nd2 = ctx.nn_search(q, c, mode, nn_mode)
            assert np.array_equal(idx[:, 0], nidx) and np.array_equal(d2[:, 0].view(np.uint32), nd2.view(np.uint32)), nn_mode
    # idx alone, and idx + count, are the same answer
    assert np.array_equal(ctx.knn_search(q, c, k, mode, want_d2=False), idx)


# ---- 2. fewer candidates than k
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k", [8, 32])
def test_fewer_candidates_than_k(ctx, k, mode):
    for m in (k - 1, k, k + 1):
        q, c = uniform_pair(40, m, 1.0)
        idx, d2, count = check(ctx, q, c, k, mode)
        assert (count == min(k, m)).all() and (idx[:, min(k, m):] == -1).all() and np.isposinf(d2[:, min(k, m):]).all()
    for m in (1, k, k + 1):
        c = uniform_pair(40, m, 1.0)[1]
        idx, d2, count = check(ctx, None, c, k, mode)
        assert (count == min(k, m - 1)).all() and (idx[:, min(k, m - 1):] == -1).all() and np.isposinf(d2[:, min(k, m - 1):]).all()


# ---- 3. ties across cell boundaries: an integer lattice, every distance exact
@functools.lru_cache(maxsize=None)
def lattice_case():
    rng = np.random.default_rng(23)
    g = np.arange(10, dtype=np.float32)
    z, y, x = np.meshgrid(g, g, g, indexing="ij")
    L = np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1)
    cloud = L[rng.permutation(1000)]
    cloud = np.concatenate([cloud, cloud[rng.integers(0, 1000, 200)]])          # 200 duplicates
    cells = L[(L < 9).all(axis=1)] + np.float32(0.5)                            # cell centres
    edges = L[L[:, 0] < 9] + np.array([0.5, 0, 0], np.float32)                  # edge midpoints
    queries = np.concatenate([L, cells, edges]).astype(np.float32)
    keys = K.sorted_keys(queries, cloud, K.DIST_CPU_ROUNDING)
    assert np.array_equal(keys, K.sorted_keys(queries, cloud, K.DIST_FMA))      # exact distances: one answer in both arithmetics
    return frozen(queries), frozen(cloud), frozen(keys)


@pytest.mark.parametrize("ppc", (None,) + CELL_REGIMES)
def test_ties_across_cell_boundaries(capi, monkeypatch, ppc):
    if ppc is not None:
        monkeypatch.setenv("MISLAM_KNN_POINTS_PER_CELL", ppc)
    queries, cloud, keys = lattice_case()
    with capi.Context(0) as c2:
        for k in (5, 6, 7, 8, 26, 27):
            for mode in MODES:
                check(c2, queries, cloud, k, mode, keys)


# ---- 4. every cell regime, from cells far smaller than the spacing to one cell for the whole cloud
@pytest.mark.parametrize("ppc", CELL_REGIMES)
def test_every_cell_regime(capi, monkeypatch, ppc):
    monkeypatch.setenv("MISLAM_KNN_POINTS_PER_CELL", ppc)
    q, c = uniform_pair(1000, 5000, 1.0)
    with capi.Context(0) as c2:
        for mode in MODES:
            check(c2, q, c, 16, mode, uniform_keys(1000, 5000, 1.0, mode))       # the same restatement in every regime: identical across them


# ---- 5. queries outside the cloud, awkward clouds
def awkward_cloud(kind):
    rng = np.random.default_rng(41)
    m = 1000
    if kind == "identical":
        return np.tile(np.array([[1.5, -2.25, 3.0]], np.float32), (m, 1))
    if kind == "collinear":
        t = rng.uniform(-5, 5, m).astype(np.float32)
        return np.stack([t, np.float32(2) * t, np.float32(-1) * t], axis=1).astype(np.float32)
    if kind == "coplanar":
        c = rng.uniform(-5, 5, (m, 3)).astype(np.float32)
        c[:, 2] = 0.75
        return c
    if kind == "two_clusters":
        c = rng.normal(scale=0.05, size=(m, 3))
        c[m // 2:] += 1e3
        return c.astype(np.float32)
    if kind == "outlier":
        c = rng.normal(scale=0.5, size=(m, 3))
        c[m - 1] = 1e6
        return c.astype(np.float32)
    assert kind == "offset"                      # fp32 spacing at 1e5 is 2^-7: many exact ties
    return (1e5 + rng.uniform(0, 1, (m, 3))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def awkward_case(kind):
    rng = np.random.default_rng(43)
    cloud = awkward_cloud(kind)
    lo, hi = cloud.min(axis=0).astype(np.float64), cloud.max(axis=0).astype(np.float64)
    diag = float(np.linalg.norm(hi - lo)) or 1.0          # (all points identical: a unit length stands in for the diagonal)
    inside = rng.uniform(lo, hi, (64, 3))
    axis, side = rng.integers(0, 3, 64), rng.integers(0, 2, 64)
    face, near = inside.copy(), inside.copy()
    face[np.arange(64), axis] = np.where(side == 0, lo[axis], hi[axis])                         # on the bounding box's faces
    near[np.arange(64), axis] = np.where(side == 0, lo[axis] - 1e-3, hi[axis] + 1e-3)           # 1e-3 outside
    d = rng.normal(size=(64, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    far10, far1e4 = inside + 10 * diag * d, inside + 1e4 * diag * d                             # 10 and 1e4 box diagonals away
    queries = np.concatenate([face, near, far10, far1e4]).astype(np.float32)
    return frozen(queries), frozen(cloud), {mode: frozen(K.sorted_keys(queries, cloud, mode)) for mode in MODES}


@pytest.mark.parametrize("kind", ["identical", "collinear", "coplanar", "two_clusters", "outlier", "offset"])
def test_queries_outside_and_awkward_clouds(ctx, kind):
    queries, cloud, keys = awkward_case(kind)
    assert queries.shape == (256, 3) and cloud.shape == (1000, 3)
    for mode in MODES:
        check(ctx, queries, cloud, 8, mode, keys[mode])
        check(ctx, None, cloud, 8, mode)


# ---- 6. self mode
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("m", [64, 1000, 5000])
def test_self_mode(ctx, m, mode):
    c = uniform_pair(1, m, 1.0)[1]
    idx, d2, count = check(ctx, None, c, 8, mode)
    assert not (idx == np.arange(m)[:, None]).any()                  # row i never contains i
    h = min(m, 1000) // 2
    twins = np.concatenate([c[:h], c[:h]])                           # every point twice: the twin comes first, at +0
    idx, d2, count = check(ctx, None, twins, 8, mode)
    assert np.array_equal(idx[:, 0], (np.arange(2 * h) + h) % (2 * h))
    assert (d2[:, 0].view(np.uint32) == 0).all() and not (idx == np.arange(len(twins))[:, None]).any()


# ---- 7. the distance limit
@pytest.mark.parametrize("mode", MODES)
def test_distance_limit(ctx, mode):
    q, c = uniform_pair(1000, 5000, 1.0)
    free = K.unpack(uniform_keys(1000, 5000, 1.0, mode), 8)
    limit = float(np.median(free[1][:, 7]))                           # half the rows are cut short
    idx, d2, count = check(ctx, q, c, 8, mode, max_d2=limit)
    assert 0 < (count < 8).sum() < 1000 and (d2[np.arange(8)[None, :] < count[:, None]] <= np.float32(limit)).all()
    # a limit of 0 keeps exact hits only
    q0 = np.concatenate([c[:100], q[:100]])
    idx, d2, count = check(ctx, q0, c, 8, mode, max_d2=0.0)
    assert (count[:100] == 1).all() and (count[100:] == 0).all() and np.array_equal(idx[:100, 0], np.arange(100))
    check(ctx, None, c[:1000], 8, mode, max_d2=limit)


# ---- 8. context hygiene
def test_a_loaded_icp_problem_survives_and_calls_do_not_leak_into_each_other(ctx, capi, golden):
    z = golden.npz("synth2k_clouds.npz")
    params = capi.icp_params(max_iterations=8)
    ctx.icp_load(z["before"], z["after"], params)
    ctx.icp_run(8)
    R0, t0, it0, err0, why0 = ctx.icp_result()
    ctx.icp_load(z["before"], z["after"], params)
    q, c = uniform_pair(1000, 5000, 1.0)
    first = ctx.knn_search(q, c, 8, K.DIST_FMA, want_count=True)
    ctx.icp_run(8)
    R1, t1, it1, err1, why1 = ctx.icp_result()
    assert it0 > 0 and (it1, why1) == (it0, why0)
    assert np.array_equal(R1.view(np.uint32), R0.view(np.uint32)) and np.array_equal(t1.view(np.uint32), t0.view(np.uint32))
    assert np.float32(err1).tobytes() == np.float32(err0).tobytes()
    # a call of another size (and k, and arithmetic) in between leaves nothing behind
    q2, c2 = uniform_pair(65, 1000, 100.0)
    ctx.knn_search(q2, c2, 32, K.DIST_CPU_ROUNDING)
    ctx.knn_search(None, c2, 3, K.DIST_CPU_ROUNDING, max_d2=1.0)
    assert same_bits(ctx.knn_search(q, c, 8, K.DIST_FMA, want_count=True), first)


# ---- 9. refusals: nothing is written
def raw_call(ctx, capi, query, n, cloud, m, k, mode=0, max_d2=np.inf, null_idx=False):
    """mi_knn_search with every output prefilled with a sentinel -> (error code, message, outputs untouched?)"""
    cap = max(n, 1) * max(min(k, 64), 1)
    idx, d2, count = np.full(cap, -7, np.int32), np.full(cap, -7.5, np.float32), np.full(max(n, 1), -7, np.int32)
    rc = capi.knn_search_raw(ctx._h, None if query is None else query.ctypes.data, n, None if cloud is None else cloud.ctypes.data, m, k, mode,
                             float(max_d2), None if null_idx else idx.ctypes.data, d2.ctypes.data, count.ctypes.data)
    return rc, capi.lib().mi_last_error().decode(), bool((idx == -7).all() and (d2 == -7.5).all() and (count == -7).all())


def test_refusals_leave_the_outputs_untouched(ctx, capi):
    q, c = (np.array(a) for a in uniform_pair(65, 1000, 1.0))
    bad_args = [
        dict(query=q, n=65, cloud=None, m=1000, k=8),                      # null cloud
        dict(query=q, n=65, cloud=c, m=1000, k=8, null_idx=True),          # null idx
        dict(query=q, n=0, cloud=c, m=1000, k=8), dict(query=q, n=-1, cloud=c, m=1000, k=8),
        dict(query=q, n=65, cloud=c, m=0, k=8),
        dict(query=q, n=65, cloud=c, m=1000, k=0), dict(query=q, n=65, cloud=c, m=1000, k=33), dict(query=q, n=65, cloud=c, m=1000, k=-1),
        dict(query=q, n=65, cloud=c, m=1000, k=8, mode=2), dict(query=q, n=65, cloud=c, m=1000, k=8, mode=-1),
        dict(query=q, n=65, cloud=c, m=1000, k=8, max_d2=float("nan")), dict(query=q, n=65, cloud=c, m=1000, k=8, max_d2=-1.0),
        dict(query=q, n=65, cloud=c, m=1000, k=8, max_d2=float("-inf")),
        dict(query=None, n=65, cloud=c, m=1000, k=8),                      # self mode with n != m
    ]
    for kw in bad_args:
        rc, msg, untouched = raw_call(ctx, capi, **kw)
        assert rc == capi.MI_ERR_INVALID_ARG and untouched and msg.startswith("mi_knn_search"), kw
    # a bad point: which array, which index -- the LOWEST one
    for value in (np.nan, np.inf, -np.inf, 1.5e18, -1.5e18):
        bc = c.copy()
        bc[917, 2] = value
        bc[333, 0] = value
        rc, msg, untouched = raw_call(ctx, capi, q, 65, bc, 1000, 8)
        assert rc == capi.MI_ERR_INVALID_ARG and untouched and "cloud_xyz point 333 " in msg, (value, msg)
        rc, msg, untouched = raw_call(ctx, capi, None, 1000, bc, 1000, 8)
        assert rc == capi.MI_ERR_INVALID_ARG and untouched and "cloud_xyz point 333 " in msg, (value, msg)
        bq = q.copy()
        bq[64, 1] = value
        bq[21, 1] = value
        rc, msg, untouched = raw_call(ctx, capi, bq, 65, c, 1000, 8)
        assert rc == capi.MI_ERR_INVALID_ARG and untouched and "query_xyz point 21 " in msg, (value, msg)
    with pytest.raises(capi.MiSlamError) as e:
        bc = c.copy()
        bc[5, 0] = np.nan
        ctx.knn_search(q, bc, 8)
    assert "cloud_xyz point 5 " in str(e.value)
    # the largest coordinates the call accepts: every distance stays finite
    big = np.array([[1e18, -1e18, 1e18], [-1e18, 1e18, -1e18], [0, 0, 0]], np.float32)
    idx, d2, count = check(ctx, big, big, 3, K.DIST_FMA)
    assert np.isfinite(d2).all()
    check(ctx, q, c, 8, K.DIST_CPU_ROUNDING, uniform_keys(65, 1000, 1.0, K.DIST_CPU_ROUNDING))     # and the context still works
