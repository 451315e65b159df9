"""GPU suite: mi_radius_search against tests/radius_reference.py, bit for bit and without a tolerance anywhere: random clouds in both
arithmetics, modes and orders; one row of every length at which the sort kernel changes its path; a row far longer than its LDS chunk;
the merged radius count and k-NN search; every cell regime; degenerate clouds; offsets beyond 2^32; the capacity protocol; refusals and
context hygiene."""
import ctypes as C
import functools

import numpy as np
import pytest

import knn_reference as K
import radius_reference as R

pytestmark = pytest.mark.gpu

MODES = (K.DIST_CPU_ROUNDING, K.DIST_FMA)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def limited(row_list, r2):
    """the rows of a larger radius cut down to the members within r2 (a row ascends by distance first)"""
    return [row[(row >> np.uint64(32)).astype(np.uint32).view(np.float32) <= np.float32(r2)] for row in row_list]


def check(got, want_rows, label, sorted_rows=True):
    """a call's (offsets, idx, d2) against the restatement's rows; unsorted rows are compared as sorted sets"""
    offsets, idx, d2 = got
    w_offsets, w_keys, w_total = R.csr(want_rows)
    assert offsets.dtype == np.int64 and np.array_equal(offsets, w_offsets), label
    assert len(idx) == w_total and len(d2) == w_total, label
    keys = R.pack(idx, d2)
    if not sorted_rows:
        keys = np.concatenate([np.sort(keys[a:b]) for a, b in zip(offsets[:-1], offsets[1:])]) if w_total else keys
    assert np.array_equal(keys, w_keys), label


# ---- 1. random clouds
@functools.lru_cache(maxsize=None)
def random_case(n, m, scale, self_mode):
    rng = np.random.default_rng(1000 * n + m + (7 if self_mode else 0))
    c = (rng.uniform(-5, 5, (m, 3)) * scale).astype(np.float32)
    q = None if self_mode else (rng.uniform(-5, 5, (n, 3)) * scale).astype(np.float32)
    # radii for mean rows of about 0.5, 8 and 40 in the bulk: density * 4/3 pi r^3 = the mean
    density = m / (10.0 * scale) ** 3
    radii = [float(np.float32((3.0 * mean / (4.0 * np.pi * density)) ** (1.0 / 3.0))) for mean in (0.5, 8.0, 40.0)]
    want = {}
    for mode in MODES:
        widest = R.rows(q, c, radii[-1], mode)
        for radius in radii:
            want[mode, radius] = limited(widest, R.r2_of(radius))
    for a in (c, q):
        if a is not None:
            a.setflags(write=False)
    return q, c, radii, want


SIZES = [(1, 1), (1, 17), (63, 5), (64, 64), (65, 1000), (1000, 333), (1000, 5000)]


@pytest.mark.parametrize("scale", [1.0, 100.0])
@pytest.mark.parametrize("n,m", SIZES)
def test_random_clouds_query_mode(ctx, capi, n, m, scale):
    q, c, radii, want = random_case(n, m, scale, False)
    for (mode, radius), rows in want.items():
        label = "n %d m %d scale %g mode %d radius %g" % (n, m, scale, mode, radius)
        check(ctx.radius_search(c, radius, q, mode, sorted=True), rows, label)
        first = ctx.radius_search(c, radius, q, mode, sorted=False)
        check(first, rows, label + " unsorted", sorted_rows=False)
        ctx.knn_search(q, c, min(3, m), mode)                                        # another call in between
        again = ctx.radius_search(c, radius, q, mode, sorted=False)
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(first, again)), label + " unsorted twice"
        idx_only = ctx.radius_search(c, radius, q, mode, sorted=True, want_d2=False)
        assert len(idx_only) == 2 and np.array_equal(idx_only[1], R.unpack(R.csr(rows)[1])[0]), label + " without d2"
    if m >= 333:
        means = [R.csr(want[K.DIST_FMA, r])[2] / n for r in radii]
        assert 0.1 < means[0] < 2 and 3 < means[1] < 12 and 12 < means[2] < 60, means      # the radii give the rows they were chosen for


@pytest.mark.parametrize("scale", [1.0, 100.0])
@pytest.mark.parametrize("m", [1, 17, 64, 65, 333, 1000])
def test_random_clouds_self_mode(ctx, capi, m, scale):
    _, c, radii, want = random_case(m, m, scale, True)
    for (mode, radius), rows in want.items():
        label = "self m %d scale %g mode %d radius %g" % (m, scale, mode, radius)
        check(ctx.radius_search(c, radius, None, mode, sorted=True), rows, label)
        first = ctx.radius_search(c, radius, None, mode, sorted=False)
        check(first, rows, label + " unsorted", sorted_rows=False)
        ctx.radius_count(c, radii[0], None, mode)
        again = ctx.radius_search(c, radius, None, mode, sorted=False)
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(first, again)), label + " unsorted twice"
        offsets, total = ctx.radius_count(c, radius, None, mode)
        assert np.array_equal(offsets, R.csr(rows)[0]) and total == R.csr(rows)[2], label + " counts only"


# ---- 2. one row of every length at an edge of the sort
def sort_edges(capi):
    w, chunk = capi.RADIUS_WAVE_ROW, capi.RADIUS_SORT_CHUNK
    fixed = [0, 1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129]
    return sorted(set(fixed + [w - 1, w, w + 1, chunk - 1, chunk, chunk + 1, 2 * chunk - 1, 2 * chunk, 2 * chunk + 1]))


def clump(length, seed):
    """a cloud with exactly `length` points within 1 of the origin, in mirror pairs p and -p (equal distance bits: the lower index first), an
    odd one on its own, among 60 points beyond 2; shuffled"""
    rng = np.random.default_rng(seed)
    half = rng.normal(size=(length // 2 + 1, 3))
    half = (half / np.linalg.norm(half, axis=1)[:, None] * rng.uniform(0.05, 0.9, (len(half), 1))).astype(np.float32)
    inside = np.concatenate([half[:length // 2], -half[:length // 2], half[length // 2:][:length % 2]])
    far = rng.normal(size=(60, 3))
    far = (far / np.linalg.norm(far, axis=1)[:, None] * rng.uniform(2.0, 4.0, (60, 1))).astype(np.float32)
    cloud = np.concatenate([inside, far]).astype(np.float32)
    return cloud[rng.permutation(len(cloud))]


def test_row_lengths_at_every_edge_of_the_sort(ctx, capi):
    q = np.array([[0, 0, 0], [40, 40, 40]], np.float32)                               # the clump's centre, and an empty row behind it
    for length in sort_edges(capi):
        cloud = clump(length, 50 + length)
        for mode in MODES:
            rows = R.rows(q, cloud, 1.0, mode)
            assert len(rows[0]) == length and len(rows[1]) == 0
            assert len(np.unique(bits(R.unpack(rows[0])[1]))) <= length // 2 + length % 2                # the ties are there
            check(ctx.radius_search(cloud, 1.0, q, mode, sorted=True), rows, "clump of %d mode %d" % (length, mode))
            check(ctx.radius_search(cloud, 1.0, q, mode, sorted=False), rows, "clump of %d mode %d unsorted" % (length, mode), sorted_rows=False)


# ---- 3. a row longer than anything staged
@functools.lru_cache(maxsize=None)
def dense_cube(m):
    c = np.random.default_rng(77).uniform(0, 0.1, (m, 3)).astype(np.float32)
    c.setflags(write=False)
    return c


def test_rows_far_longer_than_the_sorts_chunk(ctx, capi):
    c = dense_cube(5000)
    assert 4999 > 4 * capi.RADIUS_SORT_CHUNK
    rows = R.rows(None, c, 1.0, K.DIST_CPU_ROUNDING)
    assert all(len(r) == 4999 for r in rows)
    check(ctx.radius_search(c, 1.0, None, K.DIST_CPU_ROUNDING, sorted=True), rows, "5000 in a cube of 0.1")
    check(ctx.radius_search(c, 1.0, None, K.DIST_CPU_ROUNDING, sorted=False), rows, "5000 in a cube of 0.1, unsorted", sorted_rows=False)


# ---- 4. cross-checks against merged code
@pytest.mark.parametrize("mode", MODES)
def test_lengths_are_the_outlier_filters_and_heads_are_the_knn_searchs(ctx, capi, mode):
    _, c, radii, _ = random_case(1000, 1000, 1.0, True)
    q = random_case(1000, 333, 1.0, False)[0]
    for radius in radii:
        offsets, idx, d2 = ctx.radius_search(c, radius, None, mode)
        params = capi.outlier_params(method=capi.OUTLIER_RADIUS, radius=radius, min_neighbours=1, dist_mode=mode)
        neighbours = ctx.remove_outliers(c, params, want_neighbours=True)[2]
        assert np.array_equal(np.diff(offsets), neighbours.astype(np.int64)), radius
        for query, (off, ix, dd) in ((None, (offsets, idx, d2)), (q, ctx.radius_search(c, radius, q, mode))):
            lengths = np.diff(off)
            for k in (1, 8, 32):
                kidx, kd2, kcount = ctx.knn_search(query, c, k, mode, max_d2=float(R.r2_of(radius)), want_count=True)
                assert np.array_equal(kcount, np.minimum(lengths, k)), (radius, k)
                # every row's head, all rows at once: slot s of row r is entry off[r] + s where s < min(k, length), empty beyond
                slot = np.arange(k)[None, :]
                filled = slot < np.minimum(lengths, k)[:, None]
                entry = np.where(filled, off[:-1, None] + slot, 0)
                assert len(ix) > 0 or not filled.any()
                head_idx = np.where(filled, ix[entry] if len(ix) else 0, -1)
                head_d2 = np.where(filled, dd[entry] if len(dd) else 0, np.float32(np.inf)).astype(np.float32)
                assert np.array_equal(head_idx, kidx) and np.array_equal(bits(head_d2), bits(kd2)), (radius, k)


# ---- 5. cell regimes: one cell for the whole cloud, about one per radius (the default), many shells per radius
WIDE = 2.5       # a radius at which 5000 points in a box of 10 leave room for cells a quarter of it long (at most one cell per point: 17 per axis)


@functools.lru_cache(maxsize=None)
def wide_rows(self_mode):
    q, c, _, _ = random_case(1000, 1000 if self_mode else 5000, 1.0, self_mode)
    return q, c, {mode: R.rows(q, c, WIDE, mode) for mode in MODES}


@pytest.mark.parametrize("variable,value,regime", [("MISLAM_OUTLIER_RADIUS_CELL", "1024", "one"), ("MISLAM_KNN_POINTS_PER_CELL", "1e9", "one"),
                                                   ("MISLAM_OUTLIER_RADIUS_CELL", "1", "default"), ("MISLAM_OUTLIER_RADIUS_CELL", "0.25", "fine")])
def test_cell_regimes_give_the_same_rows(ctx, capi, monkeypatch, variable, value, regime):
    q, c, want = wide_rows(False)
    _, cs, want_s = wide_rows(True)
    ctx.radius_count(c, WIDE, q)
    default = ctx.radius_grid()                                                       # (the session's context: nothing set)
    assert default == (4, 4, 4), default                                              # a box of 10 in cells of 2.5
    monkeypatch.setenv(variable, value)
    with capi.Context(0) as c2:
        for mode in MODES:
            for srt in (True, False):
                check(c2.radius_search(cs, WIDE, None, mode, sorted=srt), want_s[mode], "%s=%s self mode %d" % (variable, value, mode), sorted_rows=srt)
                check(c2.radius_search(c, WIDE, q, mode, sorted=srt), want[mode], "%s=%s query mode %d" % (variable, value, mode), sorted_rows=srt)
        dims = c2.radius_grid()
    # the variable was taken and gave the regime it was set for
    if regime == "one":
        assert dims == (1, 1, 1), dims
    elif regime == "default":
        assert dims == default, (dims, default)
    else:
        assert all(d >= 15 for d in dims), dims                                      # a quarter of the edge: four shells of cells per radius


# ---- 6. degenerate clouds
def degenerate_clouds():
    rng = np.random.default_rng(9)
    t = rng.uniform(-3, 3, 300).astype(np.float32)
    plane = rng.uniform(-3, 3, (300, 3)).astype(np.float32)
    plane[:, 2] = 0.5
    outlier = rng.uniform(-1, 1, (300, 3)).astype(np.float32)
    outlier[299] = (4e5, -3e5, 2e5)
    return {"identical": np.full((300, 3), 1.25, np.float32), "collinear": np.stack([t, 2 * t, -t], axis=1).astype(np.float32), "coplanar": plane,
            "outlier": outlier, "single": np.array([[0.5, -0.25, 2.0]], np.float32)}


@pytest.mark.parametrize("kind", ["identical", "collinear", "coplanar", "outlier", "single"])
def test_degenerate_clouds(ctx, capi, kind):
    c = degenerate_clouds()[kind]
    inside = np.concatenate([c[:5] + np.float32(0.1), c[:5]])
    far = np.array([[1e6, 1e6, 1e6], [-1e6, 0, 0], [0, 0, 3e7], [500, -500, 500]], np.float32)      # far outside the cloud's box: empty rows
    q = np.concatenate([inside, far]).astype(np.float32)
    for mode in MODES:
        for radius in (0.5, 1.0):
            for srt in (True, False):
                check(ctx.radius_search(c, radius, None, mode, sorted=srt), R.rows(None, c, radius, mode), "%s self %g" % (kind, radius), sorted_rows=srt)
                rows = R.rows(q, c, radius, mode)
                got = ctx.radius_search(c, radius, q, mode, sorted=srt)
                check(got, rows, "%s queries %g" % (kind, radius), sorted_rows=srt)
                assert (np.diff(got[0])[-4:] == 0).all()
    if kind == "identical":
        offsets, idx, d2 = ctx.radius_search(c, 0.5, None)
        assert (np.diff(offsets) == 299).all() and (bits(d2) == 0).all() and idx[:299].tolist() == list(range(1, 300))


# ---- 7. offsets beyond 2^32, counts only: the expected values are analytic
def test_offsets_pass_two_to_the_32(ctx, capi):
    m = 66000
    c = dense_cube(m)
    offsets, total = ctx.radius_count(c, 1.0)
    assert total == 4355934000 == m * (m - 1) and total > 2 ** 32
    assert np.array_equal(offsets, np.arange(m + 1, dtype=np.int64) * (m - 1))


# ---- 8. the capacity protocol
def raw(ctx, capi, q, c, radius=1.0, mode=K.DIST_CPU_ROUNDING, srt=1, capacity=0, lists=True, want_d2=True, n=None, m=None, null=(), handle=True):
    """mi_radius_search with every output prefilled with a sentinel -> (code, message, offsets, idx, d2, total)"""
    n = (len(c) if q is None else len(q)) if n is None else n
    m = len(c) if m is None else m
    entries = max(int(min(capacity, 1 << 20)), 1)
    offsets, idx, d2 = np.full(max(n, 0) + 1, -7, np.int64), np.full(entries, -7, np.int32), np.full(entries, -7.5, np.float32)
    total = C.c_longlong(-7)
    rc = capi.radius_search_raw(ctx._h if handle else None, None if q is None else q.ctypes.data, n, None if "cloud" in null else c.ctypes.data, m,
                                float(radius), int(mode), int(srt), None if "offsets" in null else offsets.ctypes.data,
                                idx.ctypes.data if lists else None, d2.ctypes.data if want_d2 else None, int(capacity),
                                None if "total" in null else C.addressof(total))
    return rc, capi.lib().mi_last_error().decode(), offsets, idx, d2, total.value


def test_capacity_protocol(ctx, capi):
    q, c, radii, want = random_case(1000, 5000, 1.0, False)
    rows = want[K.DIST_CPU_ROUNDING, radii[1]]
    w_offsets, w_keys, total = R.csr(rows)
    w_idx, w_d2 = R.unpack(w_keys)
    assert total > 1000
    # one short: the lists stay untouched, the offsets and the total are right, and the call succeeds
    rc, _, offsets, idx, d2, got_total = raw(ctx, capi, q, c, radii[1], capacity=total - 1)
    assert rc == capi.MI_OK and got_total == total and np.array_equal(offsets, w_offsets) and (idx == -7).all() and (d2 == -7.5).all()
    for capacity in (total, total + 7):
        rc, _, offsets, idx, d2, got_total = raw(ctx, capi, q, c, radii[1], capacity=capacity)
        assert rc == capi.MI_OK and got_total == total and np.array_equal(offsets, w_offsets)
        assert np.array_equal(idx[:total], w_idx) and np.array_equal(bits(d2[:total]), bits(w_d2))
        assert (idx[total:] == -7).all() and (d2[total:] == -7.5).all() and len(idx) == capacity
    # the binding's own two-call form and a short bound
    with pytest.raises(capi.MiSlamError, match="%d neighbours" % total):
        ctx.radius_search(c, radii[1], q, capacity=total - 1)
    for kw, cause in ((dict(capacity=0), "capacity"), (dict(capacity=capi.RADIUS_MAX_TOTAL + 1), "capacity"), (dict(capacity=-1), "capacity"),
                      (dict(capacity=0, lists=False, want_d2=True), "d2 given without idx"), (dict(capacity=5, lists=False, want_d2=False), "capacity")):
        rc, msg, offsets, idx, d2, got_total = raw(ctx, capi, q, c, radii[1], **kw)
        assert rc == capi.MI_ERR_INVALID_ARG and msg.startswith("mi_radius_search") and cause in msg, (kw, msg)
        assert (offsets == -7).all() and (idx == -7).all() and (d2 == -7.5).all() and got_total == -7, kw


# ---- 9. contracts
def test_refusals_leave_the_outputs_untouched(ctx, capi):
    q, c, _, _ = random_case(65, 1000, 1.0, False)
    q, c = np.array(q), np.array(c)
    nan, inf = float("nan"), float("inf")
    cases = [(dict(null=("cloud",)), "null"), (dict(null=("offsets",)), "null"), (dict(null=("total",)), "null"),
             (dict(n=0), "empty"), (dict(n=-1), "empty"), (dict(m=0), "empty"), (dict(m=-5), "empty"),
             (dict(mode=2), "dist_mode"), (dict(mode=-1), "dist_mode"), (dict(srt=2), "sorted"), (dict(srt=-1), "sorted"),
             (dict(radius=nan), "radius"), (dict(radius=inf), "radius"), (dict(radius=0.0), "radius"), (dict(radius=-1.0), "radius"),
             (dict(radius=1e20), "square")]
    for kw, cause in cases:
        rc, msg, offsets, idx, d2, total = raw(ctx, capi, q, c, capacity=64, **kw)
        assert rc == capi.MI_ERR_INVALID_ARG and msg.startswith("mi_radius_search") and cause in msg, (kw, msg)
        assert (offsets == -7).all() and (idx == -7).all() and (d2 == -7.5).all() and total == -7, kw
    rc, msg, offsets, idx, d2, total = raw(ctx, capi, None, c, capacity=64, n=999)                   # self mode with n != m
    assert rc == capi.MI_ERR_INVALID_ARG and "self mode" in msg and (offsets == -7).all() and total == -7
    # a bad point is named by array and lowest index
    for array, name, rows in (("cloud", "cloud_xyz", (700, 41)), ("query", "query_xyz", (64, 3))):
        for bad in (nan, inf, -inf, 2e18):
            q2, c2 = q.copy(), c.copy()
            for r in rows:
                (c2 if array == "cloud" else q2)[r, 1] = bad
            rc, msg, offsets, idx, d2, total = raw(ctx, capi, q2, c2, capacity=64)
            assert rc == capi.MI_ERR_INVALID_ARG and msg.startswith("mi_radius_search") and "%s point %d " % (name, min(rows)) in msg, msg
            assert (offsets == -7).all() and (idx == -7).all() and (d2 == -7.5).all() and total == -7
    rc, msg, offsets, idx, d2, total = raw(ctx, capi, q, c, capacity=64, handle=False)
    assert rc == capi.MI_ERR_INVALID_ARG and "null context" in msg and (offsets == -7).all() and total == -7
    # the context is as usable as before
    check(ctx.radius_search(c, 1.0, q), R.rows(q, c, 1.0), "after the refusals")


def test_a_loaded_icp_problem_survives_and_nothing_leaks(ctx, capi, golden):
    z = golden.npz("synth2k_clouds.npz")
    params = capi.icp_params(max_iterations=8)
    ctx.icp_load(z["before"], z["after"], params)
    ctx.icp_run(8)
    R0, t0, it0, err0, why0 = ctx.icp_result()
    ctx.icp_load(z["before"], z["after"], params)
    q, c, radii, want = random_case(1000, 5000, 1.0, False)
    first = ctx.radius_search(c, radii[1], q, K.DIST_FMA)
    ctx.radius_search(z["after"], 0.5, None, sorted=False)
    ctx.icp_run(8)
    R1, t1, it1, err1, why1 = ctx.icp_result()
    assert it0 > 0 and (it1, why1) == (it0, why0)
    assert np.array_equal(bits(R1), bits(R0)) and np.array_equal(bits(t1), bits(t0)) and np.float32(err1).tobytes() == np.float32(err0).tobytes()
    # 20 calls of alternating sizes: the buffers grow once and no more
    small = random_case(65, 1000, 1.0, False)

    def alternate(i):
        qq, cc, rr, _ = (small, (q, c, radii, want))[i % 2]
        ctx.radius_search(cc, rr[1 + i % 2], qq, sorted=bool(i % 3))

    alternate(0), alternate(1)                                                        # both sizes once: every buffer has its largest length
    ctx.synchronize()
    before = capi.selftest_live_buffers()
    for i in range(20):
        alternate(i)
    ctx.synchronize()
    assert capi.selftest_live_buffers() <= before
    again = ctx.radius_search(c, radii[1], q, K.DIST_FMA)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(first, again))
    check(again, want[K.DIST_FMA, radii[1]], "after 20 calls")
