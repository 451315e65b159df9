"""GPU suite: mi_scan_context and mi_scan_context_search against tests/scan_context_reference.py, bit for bit and without a tolerance
anywhere: descriptors at every size, batch and shape, on the rule's own boundaries; the search at database sizes around one and a few
64-row units, at shapes that pad the matrix instruction's tile and K, with empty columns, duplicates, limits and the runner-up; the
planted places end to end; refusals and context hygiene.  Every database here (1 to 300 rows under 1 to 70 queries) plans one 64-row unit
per chunk on any device from 32 CUs on, so a wave walks at most 32 rows of one unit: chunks of several units, limits inside and across
them, winners in different chunks and rows beyond 2^16 are tests/test_gpu_scan_context_scale.py's."""
import ctypes as C
import functools

import numpy as np
import pytest

import scan_context_reference as S
from test_scan_context_reference import PLACES, SHAPES, planted, planted_winners

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


@functools.lru_cache(maxsize=None)
def shape_params(capi, rings, sectors, max_radius=50.0):
    params = capi.scan_context_params(rings=rings, sectors=sectors, max_radius=max_radius)
    return params, capi.scan_context_tables(params)


def cloud(seed, n):
    """n points on a square that reaches past max_radius = 50, heights on both sides of -z_offset"""
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.uniform(-60, 60, (n, 2)), rng.uniform(-6, 9, (n, 1))], axis=1).astype(np.float32)


# ---- 1. descriptors: sizes, batches, shapes
def test_descriptor_sizes(ctx, capi):
    params, tables = shape_params(capi, 20, 60)
    # one point, around a wave, several waves, more than one slice of SC_SLICE points (5 000 and SC_SLICE + 1)
    for n in (1, 63, 64, 65, 257, 5000, capi.SC_SLICE + 1):
        c = cloud(n, n)
        got = ctx.scan_context([c], params=params)
        assert got.shape == (1, 20, 60) and same(got[0], S.descriptor(c, None, params.z_offset, *tables)), n


def test_descriptor_batches(ctx, capi):
    params, tables = shape_params(capi, 20, 60)
    clouds = [cloud(11, 700), cloud(12, 5000), np.zeros((0, 3), np.float32), cloud(13, 1), cloud(14, 9000)]
    centres = np.array([[1, 2, 3], [0, 0, 0], [5, 5, 5], [-3.5, 0.25, 0], [10, -10, 1]], np.float32)
    for cen in (None, centres):
        batch = ctx.scan_context(clouds, centres=cen, params=params)
        assert same(batch, S.descriptors(clouds, cen, params, tables))
        assert (bits(batch[2]) == 0).all()                               # the empty scan: +0 everywhere
        for i, c in enumerate(clouds):                                   # a scan's descriptor does not depend on the batch
            alone = ctx.scan_context([c], centres=None if cen is None else cen[i:i + 1], params=params)
            assert same(alone[0], batch[i]), i
        assert same(ctx.scan_context(clouds, centres=cen, params=params), batch)      # the same call twice
    # the concatenated form with explicit offsets is the same call
    xyz, offsets = np.concatenate(clouds), np.cumsum([0] + [len(c) for c in clouds])
    assert same(ctx.scan_context(xyz, offsets=offsets, centres=centres, params=params), batch)


@pytest.mark.parametrize("rings,sectors", SHAPES)
def test_descriptor_shapes(ctx, capi, rings, sectors):
    params, tables = shape_params(capi, rings, sectors)
    clouds = [cloud(100 * rings + sectors + i, 3000 + 17 * i) for i in range(3)]
    centres = np.array([[0.5, -0.25, 0], [7, 7, 7], [-20, 3, -1]], np.float32)
    for cen in (None, centres):
        got = ctx.scan_context(clouds, centres=cen, params=params)
        assert got.shape == (3, rings, sectors) and same(got, S.descriptors(clouds, cen, params, tables))
        assert (got > 0).any()


# ---- 2. descriptors: the rule's own boundaries
@pytest.mark.parametrize("rings,sectors", [(4, 8), (20, 60), (7, 13)])
def test_descriptor_edge_cases(ctx, capi, rings, sectors):
    params, tables = shape_params(capi, rings, sectors, 8.0)
    edge2, dirs = tables
    radii = np.sqrt(edge2)                                               # with max_radius 8 and 4 rings: 0, 2, 4, 6, 8, exact
    on = (radii[:, None, None] * dirs[None, :, :]).reshape(-1, 2)      # every ring edge x every boundary direction, max_radius included
    rng = np.random.default_rng(rings)
    pts = np.concatenate([on, np.zeros((1, 2)), -np.zeros((1, 2)), [[8.0, 0.0], [0.0, -8.0], [9.0, 1.0], [np.nextafter(np.float32(8), 0), 0.0]]])
    pts = np.concatenate([pts, rng.uniform(0.5, 3.0, (len(pts), 1))], axis=1).astype(np.float32)
    centre = np.array([[16.0, -4.0, 0.0]], np.float32)                   # the moved points are rounded anew: other bins, the same rule
    for cen, moved in ((None, pts), (centre, pts + centre)):
        ring, sector = S.bins(moved, None if cen is None else cen[0], edge2, dirs)
        assert (ring == -1).any() and (ring[len(on)] == 0) and sector[len(on)] == 0      # max_radius is out; the centre is bin (0, 0)
        got = ctx.scan_context([moved], centres=cen, params=params)
        assert same(got[0], S.descriptor(moved, None if cen is None else cen[0], params.z_offset, edge2, dirs)), (rings, sectors)
    # heights that are negative, zero and positive after the offset; a scan whose every point is out of range
    low = pts.copy()
    low[:, 2] = np.where(np.arange(len(low)) % 3 == 0, -2.0, np.where(np.arange(len(low)) % 3 == 1, -7.0, -1.5))
    far = pts.copy()
    far[:, :2] = far[:, :2] + 100.0
    got = ctx.scan_context([low, far], params=params)
    assert same(got[0], S.descriptor(low, None, params.z_offset, edge2, dirs)) and (got[0] >= 0).all() and (got[0] == 0.5).any()
    assert (bits(got[1]) == 0).all()


# ---- 3. the search
def random_descriptors(seed, rows, rings, sectors, empty=0.2):
    rng = np.random.default_rng(seed)
    d = rng.uniform(0, 12, (rows, rings, sectors)) * (rng.uniform(0, 1, (rows, rings, sectors)) < 0.7)
    return (d * (rng.uniform(0, 1, (rows, 1, sectors)) >= empty)).astype(np.float32)


def check_search(ctx, params, query, db, limit=None, label="", want=None):
    idx, dist, shift, second = ctx.scan_context_search(query, db, limit=limit, params=params, want_second=True)
    w_idx, w_dist, w_shift, w_second = want if want is not None else S.search(query, db, limit)
    assert np.array_equal(idx, w_idx) and np.array_equal(shift, w_shift), (label, idx, w_idx, shift, w_shift)
    assert same(dist, w_dist) and same(second, w_second), (label, dist, w_dist, second, w_second)
    three = ctx.scan_context_search(query, db, limit=limit, params=params)
    assert len(three) == 3 and all(np.array_equal(a, b) for a, b in zip(three, (idx, dist, shift))), label
    return idx, dist, shift, second


def test_search_database_sizes(ctx, capi):
    # a workgroup takes a chunk of SC_SEARCH_CHUNK = 64 rows (a multiple of it); its waves take every SC_SEARCH_WAVES-th row
    chunk = capi.SC_SEARCH_CHUNK
    assert chunk == 64
    params, _ = shape_params(capi, 20, 60)
    query = random_descriptors(1, 1, 20, 60)
    for nd in (1, 63, 64, 65, chunk + 1, 2 * chunk + 1, 300):
        db = random_descriptors(1000 + nd, nd, 20, 60)
        db[nd // 2] = query[0]                                           # a planted duplicate: distance 0 to one part in 2^23, shift 0
        idx, dist, shift, _ = check_search(ctx, params, query, db, label="nd %d" % nd)
        assert idx[0] == nd // 2 and shift[0] == 0 and abs(float(dist[0])) <= 22 * 2.0 ** -24


def test_search_query_counts(ctx, capi):
    params, _ = shape_params(capi, 7, 13)
    db = random_descriptors(5, 2 * capi.SC_SEARCH_CHUNK + 1, 7, 13)
    for nq in (1, 5, 70):
        check_search(ctx, params, random_descriptors(50 + nq, nq, 7, 13), db, label="nq %d" % nq)


@pytest.mark.parametrize("rings,sectors", SHAPES)
def test_search_shapes(ctx, capi, rings, sectors):
    """60 and 13 sectors pad the 32-wide tiles, 20 and 7 rings the instruction's K and the kernel's K-steps: no padding reaches a diagonal."""
    params, _ = shape_params(capi, rings, sectors)
    db = random_descriptors(10 * rings + sectors, 70, rings, sectors)
    # three rows seen again, turned by half a turn, with a little of something else on top
    query = (np.roll(db[[3, 41, 69]], sectors // 2, axis=2) + random_descriptors(7, 3, rings, sectors, empty=0.0) * np.float32(0.05)).astype(np.float32)
    idx, dist, shift, second = check_search(ctx, params, query, db, label="%d x %d" % (rings, sectors))
    if sectors > 1:
        assert idx.tolist() == [3, 41, 69] and (second > dist).all()


def test_search_contract_cases(ctx, capi):
    params, _ = shape_params(capi, 20, 60)
    db = random_descriptors(21, 80, 20, 60)
    db[:, :, ::2] = 0                                                    # half of the columns empty
    db[17] = 0                                                           # an all-empty row
    db[60] = db[30]                                                      # duplicate rows: the lowest wins
    query = np.stack([db[30], np.zeros((20, 60), np.float32), np.roll(db[75], 7, axis=1), db[17]])
    idx, dist, shift, second = check_search(ctx, params, query, db, label="contract")
    assert idx[0] == 30 and second[0] == dist[0]                         # the duplicate is the runner-up, at the same distance
    assert (idx[1], dist[1], shift[1], second[1]) == (0, 1.0, 0, 1.0)    # an all-empty query: distance 1, shift 0, the lowest row
    assert idx[2] == 75 and shift[2] == 60 - 7
    assert (idx[3], dist[3], shift[3]) == (0, 1.0, 0)
    only_empty = check_search(ctx, params, query[:1], db[17:18], label="an all-empty row alone")
    assert (only_empty[0][0], only_empty[1][0], only_empty[2][0], only_empty[3][0]) == (0, 1.0, 0, np.inf)
    # limits: none, one row, all rows, and a mixed array (an online caller's i - 50)
    for limit in ([0, 0, 0, 0], [1, 1, 1, 1], [80, 80, 80, 80], [0, 1, 80, 31], [-5, 64, 65, 30]):
        got = check_search(ctx, params, query, db, limit=np.array(limit, np.int32), label="limit %s" % limit)
        for i, lim in enumerate(limit):
            if lim <= 0:
                assert (got[0][i], got[1][i], got[2][i], got[3][i]) == (-1, np.inf, 0, np.inf)
            else:
                assert 0 <= got[0][i] < lim
            if lim == 1:
                assert got[3][i] == np.inf


# ---- 4. end to end
def test_planted_places_end_to_end(ctx, capi):
    params, tables, places, revisits, k, w_db, w_query = planted(capi)
    db = ctx.scan_context(places, params=params)
    query = ctx.scan_context(revisits, params=params)
    assert same(db, w_db) and same(query, w_query)
    idx, dist, shift, second = check_search(ctx, params, query, db, label="planted", want=planted_winners(capi))
    assert np.array_equal(idx, np.arange(PLACES))
    off = np.mod(shift + k + 1.0 / 3.0, params.sectors)
    assert (np.minimum(off, params.sectors - off) <= 1.0).all(), (shift, k)


def test_a_turn_by_whole_sectors_comes_back_as_sectors_minus_k(ctx, capi):
    params, tables, places, revisits, k, w_db, w_query = planted(capi)
    sectors = params.sectors
    turned = []
    for kk in (0, 1, 29, 59):
        ang = kk * 2 * np.pi / sectors
        R = np.array([[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1]])
        turned.append((places[7].astype(np.float64) @ R.T).astype(np.float32))        # counter-clockwise by kk sectors
    query = ctx.scan_context(turned, params=params)
    idx, dist, shift = ctx.scan_context_search(query, w_db, params=params)
    assert idx.tolist() == [7] * 4 and shift.tolist() == [0, 59, 31, 1], (idx, shift)


# ---- 5. contracts
def test_descriptor_refusals_leave_the_output_untouched(ctx, capi):
    good = capi.scan_context_params()
    xyz = cloud(3, 300)
    offsets = np.array([0, 100, 100, 300], np.int32)
    centres = np.zeros((3, 3), np.float32)
    nan, inf = float("nan"), float("inf")

    def raw(xyz_=xyz, offsets_=offsets, n_scans=3, centres_=centres, params=good, null=(), handle=True):
        desc = np.full((3, 20, 60), -7.5, np.float32)
        ptr = lambda name, a: None if name in null or a is None else a.ctypes.data
        rc = capi.scan_context_raw(ctx._h if handle else None, ptr("xyz", xyz_), ptr("offsets", offsets_), n_scans, ptr("centres", centres_),
                                   None if "params" in null else C.addressof(params), None if "desc" in null else desc.ctypes.data)
        return rc, capi.lib().mi_last_error().decode(), desc

    def spoiled(a, rows, value, col=1):
        a = a.copy()
        a[list(rows), col] = value
        return a

    cases = [(dict(null=("xyz",)), "null"), (dict(null=("offsets",)), "null"), (dict(null=("params",)), "null"), (dict(null=("desc",)), "null"),
             (dict(n_scans=0), "n_scans"), (dict(n_scans=-2), "n_scans"),
             (dict(offsets_=np.array([1, 100, 100, 300], np.int32)), "offsets[0]"), (dict(offsets_=np.array([0, 100, 99, 300], np.int32)), "index 2"),
             (dict(offsets_=np.array([0, 200, 100, 50], np.int32)), "index 2")]
    for kw, word in ((dict(rings=0), "rings"), (dict(rings=33), "rings"), (dict(sectors=0), "sectors"), (dict(sectors=65), "sectors"),
                     (dict(max_radius=0.0), "max_radius"), (dict(max_radius=-1.0), "max_radius"), (dict(max_radius=inf), "max_radius"),
                     (dict(max_radius=nan), "max_radius"), (dict(z_offset=nan), "z_offset"), (dict(z_offset=inf), "z_offset")):
        cases.append((dict(params=capi.scan_context_params(**kw)), word))
    for bad in (nan, inf, -inf, 2e18):
        cases.append((dict(centres_=spoiled(centres, (2, 1), bad)), "centres of scan 1 "))
        cases.append((dict(xyz_=spoiled(xyz, (250, 41), bad)), "xyz point 41 "))
        cases.append((dict(xyz_=spoiled(xyz, (299,), bad, col=2)), "xyz point 299 "))
    for kw, word in cases:
        rc, msg, desc = raw(**kw)
        assert rc == capi.MI_ERR_INVALID_ARG and msg.startswith("mi_scan_context:") and word in msg, (kw, msg)
        assert (desc == -7.5).all(), kw
    rc, msg, desc = raw(handle=False)
    assert rc == capi.MI_ERR_INVALID_ARG and "null context" in msg and (desc == -7.5).all()
    rc, msg, desc = raw(centres_=None)                                    # centres may be NULL; the context is as usable as before
    assert rc == capi.MI_OK and same(desc, S.descriptors([xyz[:100], xyz[100:100], xyz[100:]], None, good, capi.scan_context_tables(good)))


def test_search_refusals_leave_the_outputs_untouched(ctx, capi):
    good = capi.scan_context_params(rings=7, sectors=13)
    query, db = random_descriptors(1, 5, 7, 13), random_descriptors(2, 70, 7, 13)
    nan, inf = float("nan"), float("inf")

    def raw(query_=query, db_=db, nq=5, nd=70, limit=None, params=good, null=(), handle=True):
        outs = dict(idx=np.full(5, -7, np.int32), dist=np.full(5, -7.5, np.float32), shift=np.full(5, -7, np.int32), second=np.full(5, -7.5, np.float32))
        ptr = lambda name, a: None if name in null or a is None else a.ctypes.data
        rc = capi.scan_context_search_raw(ctx._h if handle else None, ptr("query", query_), nq, ptr("db", db_), nd, ptr("limit", limit),
                                          None if "params" in null else C.addressof(params), ptr("idx", outs["idx"]), ptr("dist", outs["dist"]),
                                          ptr("shift", outs["shift"]), ptr("second", outs["second"]))
        untouched = (outs["idx"] == -7).all() and (outs["dist"] == -7.5).all() and (outs["shift"] == -7).all() and (outs["second"] == -7.5).all()
        return rc, capi.lib().mi_last_error().decode(), untouched, outs

    def spoiled(a, rows, value):
        a = a.copy()
        for r in rows:
            a[r, 3, 5] = value
        return a

    cases = [(dict(null=(name,)), "null") for name in ("query", "db", "params", "idx", "dist", "shift")]
    cases += [(dict(nq=0), "empty"), (dict(nq=-1), "empty"), (dict(nd=0), "empty"), (dict(nd=-3), "empty"),
              (dict(limit=np.array([70, 70, 71, 0, 72], np.int32)), "limit of query 2 "),
              (dict(params=capi.scan_context_params(rings=0, sectors=13)), "rings"), (dict(params=capi.scan_context_params(rings=7, sectors=65)), "sectors"),
              (dict(params=capi.scan_context_params(rings=7, sectors=13, max_radius=nan)), "max_radius")]
    for bad in (nan, inf, -inf, -1.0):
        cases.append((dict(query_=spoiled(query, (4, 2), bad)), "query_desc row 2 "))
        cases.append((dict(db_=spoiled(db, (69, 64, 66), bad)), "db_desc row 64 "))
    cases.append((dict(query_=spoiled(query, (1,), nan), db_=spoiled(db, (0,), nan)), "query_desc row 1 "))      # query_desc first
    for kw, word in cases:
        rc, msg, untouched, _ = raw(**kw)
        assert rc == capi.MI_ERR_INVALID_ARG and msg.startswith("mi_scan_context_search:") and word in msg, (kw, msg)
        assert untouched, kw
    rc, msg, untouched, _ = raw(handle=False)
    assert rc == capi.MI_ERR_INVALID_ARG and "null context" in msg and untouched
    rc, msg, untouched, outs = raw(null=("second", "limit"))              # both may be NULL; the context is as usable as before
    want = S.search(query, db)
    assert rc == capi.MI_OK and np.array_equal(outs["idx"], want[0]) and same(outs["dist"], want[1]) and np.array_equal(outs["shift"], want[2])
    assert (outs["second"] == -7.5).all()


def test_a_distributed_context_is_refused(capi):
    params = capi.scan_context_params(rings=7, sectors=13)
    with capi.Context(0, 0, 1, exchange=lambda array, kind: None) as dist:      # one rank over the caller's transport: distributed all the same
        with pytest.raises(capi.MiSlamError, match="error %d" % capi.MI_ERR_STATE):
            dist.scan_context([cloud(1, 50)], params=params)
        with pytest.raises(capi.MiSlamError, match="error %d" % capi.MI_ERR_STATE):
            dist.scan_context_search(random_descriptors(1, 2, 7, 13), random_descriptors(2, 3, 7, 13), params=params)


def test_a_loaded_icp_problem_survives_and_nothing_leaks(ctx, capi, golden):
    z = golden.npz("synth2k_clouds.npz")
    icp = capi.icp_params(max_iterations=8)
    ctx.icp_load(z["before"], z["after"], icp)
    ctx.icp_run(8)
    R0, t0, it0, err0, why0 = ctx.icp_result()
    ctx.icp_load(z["before"], z["after"], icp)
    params, tables, places, revisits, k, w_db, w_query = planted(capi)
    first = ctx.scan_context(places[:8], params=params)
    found = ctx.scan_context_search(w_query[:8], w_db, params=params, want_second=True)
    ctx.icp_run(8)
    R1, t1, it1, err1, why1 = ctx.icp_result()
    assert it0 > 0 and (it1, why1) == (it0, why0)
    assert same(R1, R0) and same(t1, t0) and np.float32(err1).tobytes() == np.float32(err0).tobytes()
    times = ctx.scan_context_times()
    assert set(times) == set(capi.Context._TIMES["scan_context"]) and times["total"] > 0 and all(v >= 0 for v in times.values())

    # 20 calls of alternating sizes: the buffers grow once and no more
    def alternate(i):
        n = (3, 8)[i % 2]
        ctx.scan_context(places[:n], params=params)
        ctx.scan_context_search(w_query[:n], w_db[:5 * n], params=params, want_second=bool(i % 3))

    alternate(0), alternate(1)
    ctx.synchronize()
    before = capi.selftest_live_buffers()
    for i in range(20):
        alternate(i)
    ctx.synchronize()
    assert capi.selftest_live_buffers() <= before
    assert same(ctx.scan_context(places[:8], params=params), first) and same(first, w_db[:8])
    again = ctx.scan_context_search(w_query[:8], w_db, params=params, want_second=True)
    assert all(np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32)) for a, b in zip(found, again))
