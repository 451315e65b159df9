"""Every case of tests/test_gpu_ndt_scale.py is what it is named for -- by the numpy restatements alone (ndt_reference.voxels' starts and
counts, ndt_reference.sums_at, and tests/ndt_scale_cases.py's restatement of the table for the wrap map), no device needed.  If a tile
size, the fix-up's stride, the key's layout or the hash changes, this says which case no longer tests what it claims."""
import numpy as np
import pytest

import ndt_reference as N
import ndt_scale_cases as S

TILE, WAVE = S.TILE, S.WAVE


def supported(ref_free, ref_floor):
    """what check_voxels needs of a cloud before it compares anything: without a floor no eigenvalue is raised (no voxel of coplanar
    points), and the same voxels have a distribution at both ratios"""
    assert not ref_free["raised"][ref_free["has"]].any()
    assert np.array_equal(ref_free["has"], ref_floor["has"])


def regimes(ref_floor, what, rows_above=256):
    has, raised = ref_floor["has"], ref_floor["raised"]
    assert len(has) > rows_above, (what, len(has))                              # K28's second workgroup
    assert has.any() and (~has).any(), what
    assert raised[has].any() and (~raised[has]).any(), what
    return "%s: %d rows, %d with a distribution, %d of them raised" % (what, len(has), has.sum(), raised[has].sum())


def test_run_edges():
    cloud, lengths, named = S.run_edges()
    n = len(cloud)
    refs = [N.voxels(cloud, S.RUN_EDGES_VOXEL, S.RUN_EDGES_ORIGIN, eig_ratio=r) for r in (1e-30, 0.01)]
    supported(*refs)
    count = refs[0]["count"].astype(np.int64)
    assert np.array_equal(count, lengths) and (refs[0]["coord"][:, 0] == np.arange(len(lengths))).all() and (refs[0]["coord"][:, 1:] == 0).all()
    assert np.array_equal(refs[0]["has"], count >= 6)                            # every run meant to have a covariance has one
    start = S.starts_of(count)
    end = start + count - 1
    s, e = start % TILE, end % TILE
    first_tile, last_tile = start // TILE, end // TILE
    assert 39000 < n < 41000 and n % TILE != 0

    def at(name, k=0):
        return named[name] + k

    # a run that starts at tile_lo and ends on lane 255: it spans a tile exactly
    i = at("a tile exactly")
    assert (s[i], e[i], count[i]) == (0, TILE - 1, TILE)
    # a run of 255 from a tile's edge, and 7 that start on lane 255 and end in the next tile
    i = at("255 then 7")
    assert (s[i], e[i]) == (0, TILE - 2) and (s[i + 1], count[i + 1]) == (TILE - 1, 7) and last_tile[i + 1] == first_tile[i + 1] + 1
    # 250 inside a tile; 7 across an edge; 511 that enter a tile, span it, and end on lane 0 of the next
    i = at("250, 7, 511")
    assert count[i:i + 3].tolist() == [250, 7, 511] and first_tile[i] == last_tile[i] and last_tile[i + 1] == first_tile[i + 1] + 1
    assert e[i + 2] == 0 and last_tile[i + 2] == first_tile[i + 2] + 2 and s[i + 2] == 2
    assert ((e == 0) & (count > 1)).any()                                        # (a run that enters a tile and ends on its lane 0)
    # four runs of a wave each, on the waves of one tile
    i = at("four waves")
    assert count[i:i + 4].tolist() == [WAVE] * 4 and (start[i:i + 4] % WAVE == 0).all() and s[i] == 0
    # 63 (a wave less its last lane), 130 from lane 63 over two wave edges, one point alone
    i = at("63, 130, 1")
    assert count[i:i + 3].tolist() == [63, 130, 1] and start[i] % WAVE == 0 and start[i + 1] % WAVE == WAVE - 1 and first_tile[i] == last_tile[i + 2]
    # the long run: the fix-up adds the fronts of the tiles first + 1 .. last, 64 per trip -- more than 64 of them here
    i = at("long")
    assert count[i] == 16384 + 300 and last_tile[i] - first_tile[i] > S.FIXUP_LANES
    assert (last_tile - first_tile > S.FIXUP_LANES).sum() == 1 and (last_tile - first_tile).max() == 65
    # a run that starts inside a tile and ends on its lane 255
    i = at("to lane 255 from inside")
    assert s[i] > 0 and e[i] == TILE - 1 and first_tile[i] == last_tile[i]
    # the tail: the last run enters the last, partial tile and ends at n - 1
    i = at("tail")
    assert i == len(count) - 1 and end[i] == n - 1 and count[i] >= 6 and first_tile[i] == last_tile[i] - 1 and last_tile[i] == (n - 1) // TILE
    # and between them: runs that end on every lane one workgroup's four waves begin and end with
    assert set((e % WAVE).tolist()) >= {0, WAVE - 1} and set((s % WAVE).tolist()) >= {0, WAVE - 1}
    print("run edges: %d points, %d runs, %d of them across a tile edge" % (n, len(count), (last_tile > first_tile).sum()))


@pytest.mark.parametrize("n,shifted", [(S.SORT_ONE_PASS + 1, False), (70001, False), (70001, True)])
def test_uniform_clouds(n, shifted):
    cloud, voxel, origin = S.uniform_case(n, shifted)
    assert cloud.shape == (n, 3) and n > 65536
    refs = [N.voxels(cloud, voxel, origin, eig_ratio=r) for r in (1e-30, 0.01)]
    supported(*refs)
    print(regimes(refs[1], "uniform %d%s" % (n, " shifted" if shifted else "")))
    count = refs[1]["count"]
    if n > S.SORT_ONE_PASS:
        assert n == 4096 * 64 + 1 and 8000 <= len(count) <= 9300
    if shifted:
        # the fp32 mean is coarse out there: a grain of 6e-5 at 1000, against 1e-7 of a voxel's own extent about the origin
        assert np.abs(cloud).max(axis=0).tolist() > [990, 490, 240] and np.spacing(np.float32(1000)) > 100 * np.spacing(np.float32(0.4))
        plain = N.voxels(S.uniform_case(n)[0], voxel, S.uniform_case(n)[2], eig_ratio=0.01)
        assert abs(len(plain["count"]) - len(count)) < 0.01 * len(count)          # the same scene, up to the rounding of the shift


@pytest.mark.parametrize("which", range(len(S.SORT_PATH_EXTENTS)))
def test_sort_path_clouds(which):
    for turn in range(3):
        cloud, voxel, origin, extents = S.sort_path_case(which, turn)
        assert len(cloud) <= 50000
        refs = [N.voxels(cloud, voxel, origin, eig_ratio=r) for r in (1e-30, 0.01)]
        supported(*refs)
        print(regimes(refs[1], "extents %s" % (extents,)))
        coord = refs[1]["coord"].astype(np.int64)
        span = coord.max(axis=0) - coord.min(axis=0) + 1
        assert (span <= np.array(extents)).all() and span[int(np.argmax(extents))] == max(extents)
        # the path the voxel front takes (csrc/voxel_api.hip): one packed key, or a sort per axis of 10 or 20 bits
        packed = (span <= S.PACKED_EXTENT).all()
        assert packed == (max(extents) <= S.PACKED_EXTENT) and (span <= S.MAX_EXTENT).all()
        if max(extents) == S.MAX_EXTENT:
            assert span.max() == S.MAX_EXTENT                                        # the limit itself, admitted


def test_the_restated_table_on_keys_known_by_hand():
    assert [S.table_capacity(nv) for nv in (1, 2, 3, 4, 5, 1024, 1025)] == [2, 4, 8, 8, 16, 2048, 4096]
    coord = np.array([[5, -2, 7], [6, -2, 7], [5, -1, 7], [5, -2, 8]])
    assert S.table_keys(coord).tolist() == [0, 1, 1 << 20, 1 << 40]
    # splitmix64 from the state 0: the first output is the finaliser of the increment 0x9e3779b97f4a7c15
    assert S.table_hash([0x9e3779b97f4a7c15])[0] == 0xe220a8397b1dcdaf and S.table_hash([0])[0] == 0


def neighbour_regimes(vox, queries, what):
    """queries whose own voxel lies on either face of the listed box on every axis (a neighbour at rx = -1 and at rx = ext), one and two
    voxels outside it, and in unlisted voxels inside it"""
    coord = vox["coord"].astype(np.int64)
    lo, hi = coord.min(axis=0), coord.max(axis=0)
    c, ok = N.voxel_index(queries, vox["origin"], vox["voxel"])
    assert ok.all(), what
    inside = ((c >= lo) & (c <= hi)).all(axis=1)
    listed = set(map(tuple, coord.tolist()))
    is_listed = np.array([tuple(v) in listed for v in c.tolist()])
    assert (inside & is_listed).sum() >= 500 and (inside & ~is_listed).sum() >= min(50, 10 * ((hi - lo + 1).prod() - len(coord))), what
    for a in range(3):
        others = np.delete(np.arange(3), a)
        within = ((c[:, others] >= lo[others]) & (c[:, others] <= hi[others])).all(axis=1)
        for edge, step in ((lo[a], -1), (hi[a], 1)):
            for k in (0, 1, 2):
                assert (within & (c[:, a] == edge + k * step)).any(), (what, a, step, k)
    return c, inside, is_listed


@pytest.mark.parametrize("name", S.MAP_CASES)
def test_map_cases(name):
    vox, queries = S.map_case(name)
    coord = vox["coord"].astype(np.int64)
    nv = len(coord)
    assert len(queries) <= 5000
    # the list as mi_ndt_system admits it: strictly ascending by (cz, cy, cx), every matrix positive definite with cond <= 100 (a little
    # above it behind the rounding to fp32), every mean within 0.4 voxel of its voxel's centre (plus the mean's own fp32 grain)
    key = [tuple(v[::-1]) for v in coord.tolist()]
    assert key == sorted(set(key))
    has = N.has_distribution(vox)
    lam = np.linalg.eigvalsh(N.G.full(vox["icov"].astype(np.float64))[has])
    assert (lam[:, 0] > 0).all() and (lam[:, 2] / lam[:, 0]).max() <= 100 * (1 + 1e-5)
    centre = vox["origin"].astype(np.float64) + (coord + 0.5) * vox["voxel"]
    assert (np.abs(vox["mean"] - centre) <= 0.4 * vox["voxel"] + np.spacing(np.abs(vox["mean"]))).all()
    ext = coord.max(axis=0) - coord.min(axis=0) + 1
    assert (ext <= S.MAX_EXTENT).all()

    kind = name.split()[0]
    c, inside, is_listed = neighbour_regimes(vox, queries, name) if kind != "far" else (None, None, None)
    if kind == "count":
        assert nv == int(name.split()[1]) and (coord.min(axis=0) < 0).any()
        assert (S.table_capacity(nv) == 2 * nv) == (nv in (1, 2, 4, 1024))         # a power of two: the load is exactly one half
        assert (~has).any() == (nv == 1025)
    if kind == "slab":
        axis = "xyz".index(name.split()[1])
        assert ext[axis] == S.MAX_EXTENT and coord[:, axis].min() == -2 ** 19 and coord[:, axis].max() == 2 ** 19 - 1 and (coord.min(axis=0) < 0).all()
        ends = (coord[:, axis] < -2 ** 19 + 8).sum(), (np.abs(coord[:, axis]) < 8).sum(), (coord[:, axis] >= 2 ** 19 - 8).sum()
        assert 400 <= ends[0] <= 512 and 0 < ends[1] <= 256 and 400 <= ends[2] <= 512
        keys = S.table_keys(coord)
        field = (keys >> np.uint64(20 * axis)) & np.uint64(0xfffff)
        assert len(np.unique(keys)) == nv and field.max() == 2 ** 20 - 1 and int(keys.max()).bit_length() == (43, 43, 60)[axis]      # key bits up to 59 on z
        # a field one bit short would fold the axis' bit 19 into the next field: this list then holds equal keys
        if axis < 2:
            short = [(0, 19, 40), (0, 20, 39)][axis]
            assert len(np.unique(S.table_keys(coord, short))) < nv
        else:
            assert len(np.unique(S.table_keys(coord, (0, 20, 39)))) == nv          # (z is the last field: the y slab is the one that sees << 39)
    if kind == "far":
        axis = "xyz".index(name.split()[1])
        assert coord[:, axis].min() == S.FAR_LOW == -2 ** 30 + 8 and np.abs(queries).max() < 1e18 and np.abs(vox["mean"]).max() < 1e18
        c, ok = N.voxel_index(queries, vox["origin"], vox["voxel"])
        assert ok.all() and (c[:, axis] % 64 == 0).all()
        lo, hi = coord.min(axis=0), coord.max(axis=0)
        assert c[:, axis].min() == -2 ** 30 and c[:, axis].max() > hi[axis] + 64
        for a in range(3):
            if a != axis:
                assert {lo[a] - 2, lo[a] - 1, lo[a], hi[a], hi[a] + 1, hi[a] + 2} <= set(c[:, a].tolist())
        near = ((c >= lo - 1) & (c <= hi + 1)).all(axis=1)
        assert near.sum() >= 1000 and (~near).sum() >= 100
    if kind == "wrap":
        vox2, queries2, rows = S.wrap_map()
        assert vox2 is vox and nv == S.WRAP_NV and has.all()
        mask = S.table_capacity(nv) - 1
        home = S.table_hash(S.table_keys(coord)) & np.uint64(mask)
        assert mask == 2047 and np.array_equal(np.flatnonzero(home == np.uint64(mask)), rows) and len(rows) >= 3
        # whatever order the lanes arrive in, one of those rows at most holds the last slot and the others go past it
        rng = np.random.default_rng(7)
        for order in (np.arange(nv), np.arange(nv)[::-1], rng.permutation(nv), rng.permutation(nv)):
            slot_of, wrapped = S.table_build(vox, order)
            assert wrapped >= 2 and len(set(slot_of.tolist())) == nv
        # lookups of absent keys that begin at the last slot: the unlisted cells of the box that hash there
        absent = np.flatnonzero(inside & ~is_listed)
        absent = absent[(S.table_hash(S.table_keys(c[absent], cmin=coord.min(axis=0))) & np.uint64(mask)) == np.uint64(mask)]
        assert len(absent) >= 5

    # what the restatement makes of the queries: own voxels found and not found, neighbours alone, nothing at all
    for nb in S.NEIGHBOURHOODS:
        ref = S.map_reference(name, nb)
        idx, terms = ref["idx"], ref["terms"].astype(np.int64)
        assert (idx >= 0).sum() >= 300 and (terms == 0).sum() >= 100, (name, nb)
        assert ref["sums"][28] == (terms > 0).sum() and ref["sums"][29] == terms.sum()
        if nb > 1 and nv > 1:
            assert ((idx < 0) & (terms > 0)).any() and terms.max() > 1, (name, nb)
        if nb == 27 and nv >= 1024:
            assert terms.max() >= 10
        assert (np.abs(ref["sums"][:28]) > 0).all() and np.isfinite(ref["sums"]).all()
        print("%s neighbourhood %d: %d queries, %d in a listed voxel, %d with a term, %d terms, at most %d" % (
            name, nb, len(queries), (idx >= 0).sum(), (terms > 0).sum(), terms.sum(), terms.max()))


def test_refused_positions():
    from test_gpu_plane import scene
    moving, fixed = scene("origin")[:2]
    vox = N.voxels(fixed, 0.5)
    cloud, T, out = S.refused_case(moving, vox)
    assert np.abs(cloud).max() <= 1e18 and np.isfinite(T).all() and len(out) == len(cloud) // 3 == 1000
    assert N.voxel_index(cloud, vox["origin"], 0.5)[1].all()                       # every point itself has a voxel index
    q = N.P.move_f32(T[:3, :3], T[:3, 3], cloud)
    ok = N.voxel_index(q, vox["origin"], 0.5)[1]
    assert np.array_equal(np.flatnonzero(~ok), out) and (q[out, 0] == 2.0 ** 29).all()
    for nb in S.NEIGHBOURHOODS:
        ref = N.system(cloud, vox, T[:3, :3].astype(np.float64), T[:3, 3].astype(np.float64), nb)
        assert (ref["idx"][out] == -1).all() and (ref["terms"][out] == 0).all()
        rest = np.setdiff1d(np.arange(len(cloud)), out)
        assert (ref["idx"][rest] >= 0).sum() > 1500 and ref["sums"][28] > 1500
