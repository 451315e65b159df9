"""CPU suite: tests/scan_context_reference.py, the numpy restatement of mi_scan_context and mi_scan_context_search, against its independent
plain-float64 twin (arctan2, sqrt, np.dot), and on the planted places every later test shares: the bins are identical away from the edges,
the distances agree within the fp32 chain's bound, the winners agree wherever the twin can tell them apart, and every revisit is found at the
documented shift.  The tables come from the library's host function through the binding; no device is needed."""
import functools

import numpy as np
import pytest

import scan_context_reference as S

SHAPES = [(20, 60), (1, 1), (32, 64), (7, 13)]
PLACES = 40


def bound(rings):
    """|restatement - twin| of a distance: a chain of `rings` fp32 products of numbers at most 1, each step within 2^-24 of the exact one, plus
    the roundings of the two normalisations; twice that to be safe against the mean's own rounding."""
    return 2 * (rings + 2) * 2.0 ** -24


@functools.lru_cache(maxsize=None)
def planted(capi_module):
    """(params, tables, places, revisits, k): 40 places and each of them seen again, turned by k + 1/3 sectors"""
    capi = capi_module
    params = capi.scan_context_params()
    tables = capi.scan_context_tables(params)
    rng = np.random.default_rng(2018)
    places = [S.place(rng) for _ in range(PLACES)]
    k = rng.integers(0, params.sectors, PLACES)
    revisits = [S.revisit(rng, p, params.sectors, int(kk)) for p, kk in zip(places, k)]
    db = S.descriptors(places, None, params, tables)
    query = S.descriptors(revisits, None, params, tables)
    for a in (db, query):
        a.setflags(write=False)
    return params, tables, places, revisits, k, db, query


@functools.lru_cache(maxsize=None)
def planted_winners(capi_module):
    """S.search of the planted revisits among the planted places: computed once, shared with the GPU suite"""
    params, tables, places, revisits, k, db, query = planted(capi_module)
    return S.search(query, db)


def test_the_tables_are_what_the_header_says(capi):
    for rings, sectors in SHAPES:
        params = capi.scan_context_params(rings=rings, sectors=sectors, max_radius=37.5)
        edge2, dirs = capi.scan_context_tables(params)
        assert edge2.shape == (rings + 1,) and dirs.shape == (sectors, 2)
        assert edge2[0] == 0 and edge2[-1] == 37.5 ** 2 and (np.diff(edge2) > 0).all()
        assert np.array_equal(edge2[:-1], ((37.5 * np.arange(rings)) / rings) ** 2)
        ang = 2 * np.pi * np.arange(sectors) / sectors
        # two roundings of an angle below 2 pi on either side (a product and a quotient, ulp(2 pi) = 8.9e-16), carried through cos and sin
        assert np.abs(dirs[:, 0] - np.cos(ang)).max() <= 4e-15 and np.abs(dirs[:, 1] - np.sin(ang)).max() <= 4e-15
        assert tuple(dirs[0]) == (1.0, 0.0)
        if sectors % 2 == 0:
            assert np.array_equal(dirs[sectors // 2:], -dirs[:sectors // 2])
        if sectors % 4 == 0:
            assert tuple(dirs[sectors // 4]) == (0.0, 1.0)


@pytest.mark.parametrize("rings,sectors", SHAPES)
def test_bins_equal_the_twins_away_from_the_edges(capi, rings, sectors):
    params = capi.scan_context_params(rings=rings, sectors=sectors, max_radius=50.0)
    edge2, dirs = capi.scan_context_tables(params)
    rng = np.random.default_rng(100 * rings + sectors)
    for centre in (None, np.array([3.25, -7.5, 1.0], np.float32)):
        xyz = rng.uniform(-60, 60, (4000, 3)).astype(np.float32)
        # the test's own inputs: no point within 1e-9 (relative) of a ring edge or a sector boundary, so nothing is left out below
        assert S.boundary_margin(xyz, centre, rings, sectors, 50.0) > 1e-9
        ring, sector = S.bins(xyz, centre, edge2, dirs)
        t_ring, t_sector = S.bins_twin(xyz, centre, rings, sectors, 50.0)
        assert np.array_equal(ring, t_ring)
        assert np.array_equal(sector[ring >= 0], t_sector[ring >= 0])
        assert (ring == -1).any() and (ring == rings - 1).any() and len(np.unique(sector)) == sectors
        got = S.descriptor(xyz, centre, params.z_offset, edge2, dirs)
        want = S.descriptor_twin(xyz, centre, rings, sectors, 50.0, params.z_offset)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_the_bins_rule_on_its_boundaries(capi):
    params = capi.scan_context_params(rings=4, sectors=8, max_radius=8.0)
    edge2, dirs = capi.scan_context_tables(params)
    pts = np.array([[0, 0, 0], [2, 0, 0], [0, 2, 0], [-2, 0, 0], [0, -2, 0], [8, 0, 0], [-0.0, -0.0, 0], [1, 2, 0], [7.99, 0, 0], [4, -0.0, 0]], np.float32)
    ring, sector = S.bins(pts, None, edge2, dirs)
    # the centre: ring 0, sector 0; an exact edge: the ring outside; an exact boundary: the sector that begins there; max_radius: out
    assert ring.tolist() == [0, 1, 1, 1, 1, -1, 0, 1, 3, 2]
    assert sector.tolist() == [0, 0, 2, 4, 6, 0, 0, 1, 0, 0]


@pytest.mark.parametrize("rings,sectors", SHAPES)
def test_distances_agree_with_the_twin_within_the_chains_bound(rings, sectors):
    rng = np.random.default_rng(7 * rings + sectors)
    db = (rng.uniform(0, 10, (12, rings, sectors)) * (rng.uniform(0, 1, (12, 1, sectors)) < 0.8)).astype(np.float32)
    query = (rng.uniform(0, 10, (3, rings, sectors)) * (rng.uniform(0, 1, (3, 1, sectors)) < 0.8)).astype(np.float32)
    uq, mq = S.unit_columns(query)
    uc, mc = S.unit_columns(db)
    worst = 0.0
    for i in range(len(query)):
        got = S.shift_distances(uq[i], mq[i], uc, mc)
        want = S.shift_distances_twin(query[i], db)
        assert got.dtype == np.float32 and got.shape == (12, sectors)
        worst = max(worst, float(np.abs(got.astype(np.float64) - want).max()))
    print("rings %d sectors %d: worst |restatement - twin| = %.3g, bound %.3g" % (rings, sectors, worst, bound(rings)))
    assert worst <= bound(rings)


def test_empty_columns_and_rows():
    db = np.zeros((3, 4, 6), np.float32)          # four rings of ones: a norm of 2, every product exact
    db[1, :, :3] = 1.0
    db[2] = db[1]
    q = np.zeros((2, 4, 6), np.float32)
    q[1, :, 3:] = 2.0
    idx, dist, shift, second = S.search(q, db)
    # an all-empty query: distance 1 everywhere, the lowest row, shift 0; a half-empty one meets the duplicate rows at the lowest row, and at
    # the lowest shift at which any of its columns meets a non-empty one (shift 1: its column 5 on the row's column 0; shift 3 aligns all three)
    assert idx.tolist() == [0, 1] and dist.tolist() == [1.0, 0.0] and shift.tolist() == [0, 1] and second.tolist() == [1.0, 0.0]
    idx, dist, shift, second = S.search(q, db, limit=[0, 1])
    assert idx.tolist() == [-1, 0] and dist.tolist() == [np.inf, 1.0] and shift.tolist() == [0, 0] and second.tolist() == [np.inf, np.inf]


def test_every_planted_revisit_is_found_at_the_documented_shift(capi):
    params, tables, places, revisits, k, db, query = planted(capi)
    sectors = params.sectors
    idx, dist, shift, second = planted_winners(capi)
    assert np.array_equal(idx, np.arange(PLACES)), (idx, dist)
    # the query is the place turned counter-clockwise by k + 1/3 sectors: turning it on by `shift` sectors must bring it back, to a sector
    off = np.mod(shift + k + 1.0 / 3.0, sectors)
    assert (np.minimum(off, sectors - off) <= 1.0).all(), (shift, k)
    assert (second > dist).all()
    # the twin: the same winners, told apart by more than twice the bound at every planted query -- so the restatement is never excused
    for i in range(PLACES):
        t = S.shift_distances_twin(query[i], db).min(axis=1)
        order = np.sort(t)
        assert order[1] - order[0] > 2 * bound(params.rings), i
        assert int(t.argmin()) == idx[i]
        assert abs(float(dist[i]) - order[0]) <= bound(params.rings)


def test_descriptors_of_the_planted_places_equal_the_twins(capi):
    params, tables, places, revisits, k, db, query = planted(capi)
    checked = 0
    for cloud, got in list(zip(places, db))[:6] + list(zip(revisits, query))[:6]:
        if S.boundary_margin(cloud, None, params.rings, params.sectors, params.max_radius) > 1e-9:
            want = S.descriptor_twin(cloud, None, params.rings, params.sectors, params.max_radius, params.z_offset)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
            checked += 1
    assert checked == 12
