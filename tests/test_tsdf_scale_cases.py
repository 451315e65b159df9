"""CPU suite: every case of tests/tsdf_scale_cases.py is what it is named for, shown with tests/tsdf_reference.py alone -- the extents of the
wide maps and of the three exact edges, the coordinate ranges of the far ones, the empty runs of the thousand scans and what a scan index
off by one does to their map, the ray and tile counts of the many-rays cases, the length of the long runs and the fp32 roundings of the
stored weights.  Each case's extents, coordinate range, longest run and reference time are printed."""
import numpy as np
import pytest

import tsdf_reference as R
import tsdf_scale_cases as S
from test_tsdf_reference import bits, same_map


def describe(key, m, run=None):
    coord = m[0].astype(np.int64)
    print("%-22s %7d voxels, extents %s, coordinates %d .. %d%s, reference %.2f s"
          % (S.ident(key), len(coord), S.extents(coord), coord.min(), coord.max(), "" if run is None else ", longest run %d" % run, S.REFERENCE_SECONDS[key]))
    assert S.REFERENCE_SECONDS[key] < 10.0
    R.check_map(*m)


@pytest.mark.parametrize("axes", S.WIDE_AXES)
def test_wide_maps_are_wide_along_the_named_axes_alone(axes):
    c = S.wide(axes)
    m = S.reference("wide", axes)
    describe(("wide", axes), m, S.longest_run(c))
    assert len(c["scans"]) == 3 and all(len(s) == 300 for s in c["scans"])
    for k, extent in enumerate(S.extents(m[0])):
        assert (extent > S.SORT_EXTENT) if "xyz"[k] in axes else (extent < 100), (axes, k, extent)
    assert not np.array_equal(S.ten_bit_order(m[0]), np.arange(len(m[0])))      # ten bits of a key would not sort this map
    # the shells are apart: scan by scan onto the map so far, every voxel still has one scan's samples alone and the map is the same
    step = None
    for s, T in zip(c["scans"], c["poses"]):
        step = S.integrate(c, scans=[s], poses=[T], map=step)
    assert same_map(step, m)


@pytest.mark.parametrize("extent", [S.SORT_EXTENT, S.SORT_EXTENT + 1, S.MAX_EXTENT])
def test_edge_maps_have_their_extent_exactly(extent):
    c = S.edge(extent)
    m = S.reference("edge", extent)
    describe(("edge", extent), m)
    assert S.extents(m[0])[0] == extent and max(S.extents(m[0])[1:]) < 100
    stored = c["map"][0]
    own = R.integrate(c["scans"], c["poses"], c["origin"], c["voxel"], c["tau"])
    assert len(own[0]) > 100 and stored[0, 0] < own[0][:, 0].min() and own[0][:, 0].max() < stored[1, 0]       # strictly between the stored rows
    assert len(m[0]) == len(own[0]) + 2                      # which pass through, untouched
    line = (m[0][:, 1:] == stored[0, 1:]).all(axis=1)
    assert line.sum() >= 3                                   # a voxel of the shell lies between them in the map's order
    assert np.array_equal(S.ten_bit_order(m[0]), np.arange(len(m[0]))) == (extent == S.SORT_EXTENT)        # ten bits sort 1024 and no more
    rows = [int(np.nonzero((m[0] == r).all(axis=1))[0][0]) for r in stored]
    assert np.array_equal(bits(m[1][rows]), bits(c["map"][1])) and np.array_equal(bits(m[2][rows]), bits(c["map"][2]))


@pytest.mark.parametrize("sign", ["plus", "minus", "mixed"])
def test_far_maps_lie_beyond_two_to_the_29(sign):
    c = S.far(sign)
    m = S.reference("far", sign)
    run = S.longest_run(c)
    describe(("far", sign), m, run)
    coord = m[0].astype(np.int64)
    assert coord.min() >= -S.LIMIT and coord.max() < S.LIMIT
    lo, hi = coord.min(axis=0), coord.max(axis=0)
    want = {"plus": (1, 1, 1), "minus": (-1, -1, -1), "mixed": (1, -1, 0)}[sign]
    for k, s in enumerate(want):
        if s > 0:
            assert lo[k] >= 1 << 29
        elif s < 0:
            assert hi[k] < -(1 << 29)
        else:
            assert lo[k] < 0 < hi[k] and max(-lo[k], hi[k]) < 1000
    assert run >= 100 and len(m[0]) > len(c["map"][0])       # the samples collapse, and still reach voxels outside the stored block


def test_far_poses_lie_a_million_voxels_out():
    m = S.reference("far_poses")
    describe(("far_poses",), m, S.longest_run(S.far_poses()))
    coord = m[0].astype(np.int64)
    assert coord[:, 0].min() > 0.99e6 and coord[:, 1].max() < -0.99e6 and coord[:, 2].min() > 0.49e6
    assert max(S.extents(coord)) < 100 and len(coord) > 5000


def test_many_scans_have_their_empty_runs_and_need_their_own_poses():
    c = S.many_scans(True)
    m = S.reference("many_scans", True)
    describe(("many_scans", True), m, S.longest_run(c))
    n = np.array([len(s) for s in c["scans"]])
    assert len(n) == len(c["poses"]) == S.MANY_SCANS == 1000
    empty = np.nonzero(n == 0)[0]
    runs = np.split(empty, np.nonzero(np.diff(empty) > 1)[0] + 1)
    assert [(int(r[0]), len(r)) for r in runs] == [(0, 3), (200, 1), (400, 2), (600, 17), (997, 3)]
    assert set(n[n > 0]) == {1, 2, 3}
    t = np.array([T[:3, 3] for T in c["poses"]])
    assert np.linalg.norm(np.diff(t, axis=0), axis=1).min() > c["voxel"]
    # every ray's scan index one too low: scan s under the pose of scan s - 1
    shifted = S.integrate(c, poses=[c["poses"][0]] + c["poses"][:-1])
    assert not same_map(shifted, m) and not np.array_equal(shifted[0], m[0])
    # ... and that of the rays alone that follow an empty scan
    after = [s for s in range(1, S.MANY_SCANS) if n[s] > 0 and n[s - 1] == 0]
    assert len(after) == 4
    poses = list(c["poses"])
    for s in after:
        poses[s] = c["poses"][s - 1]
    assert not np.array_equal(S.integrate(c, poses=poses)[0], m[0])
    # the same offsets without poses: every scan in one frame
    bare = S.many_scans(False)
    assert bare["poses"] is None and [len(s) for s in bare["scans"]] == list(n)
    describe(("many_scans", False), S.reference("many_scans", False), S.longest_run(bare))


@pytest.mark.parametrize("extra", [1, 0])
def test_many_rays_fill_more_than_256_tiles(extra):
    c = S.many_rays(extra)
    m = S.reference("many_rays", extra)
    rays = len(c["scans"][0])
    samples = len(R.samples(c["scans"], None, c["origin"], c["voxel"], c["tau"])[0])
    describe(("many_rays", extra), m)
    tiles = -(-rays // S.SCAN_TILE)
    print("%d rays, %d tiles, %d surviving samples" % (rays, tiles, samples))
    assert R.half_steps(c["voxel"], c["tau"]) == 1 and rays == 256 * 1024 + extra and tiles == S.SCAN_LANES + extra
    # three samples a ray half a voxel apart: the first and the last lie a voxel apart, so a ray has two voxels at the least unless its
    # direction is far from every axis, and the band of half a voxel keeps a voxel whose centre is near the ray: more than one a ray
    assert rays < samples <= 3 * rays


@pytest.mark.parametrize("split", [False, True])
def test_long_runs_are_long(split):
    c = S.long_runs(split)
    m = S.reference("long_runs", split)
    run = S.longest_run(c)
    describe(("long_runs", split), m, run)
    assert sum(len(s) for s in c["scans"]) == S.LONG_RAYS and len(c["scans"]) == (S.LONG_SCANS if split else 1)
    assert run >= 1000 and m[2].max() == run


def test_stored_weights_round_as_stated():
    c = S.weights(None)
    m = S.reference("weights", None)
    describe(("weights", None), m, S.longest_run(c))
    coord, D, W = c["map"]
    C = S.weight_counts()
    assert np.array_equal(m[0], coord) and C.min() >= 1 and C.max() >= 3
    for w in S.STORED_WEIGHTS:
        for d in S.STORED_VALUES:
            assert ((W == np.float32(w)) & (bits(D) == bits(np.float32(d)))).any(), (w, d)        # every pair lies under samples
    one = C == 1
    big = W == np.float32(2.0 ** 24)
    assert (big & one).any() and (m[2][big & one] == np.float32(2.0 ** 24)).all()               # 2^24 + 1 rounds back
    assert (big & ~one).any() and (m[2][big & ~one] > np.float32(2.0 ** 24)).all()              # 2^24 + 2 does not
    assert np.array_equal(m[2][W == np.float32(0.5)], (C[W == np.float32(0.5)] + 0.5).astype(np.float32))
    assert np.array_equal(m[2][W == np.float32(1e-30)], C[W == np.float32(1e-30)].astype(np.float32))        # the stored weight is lost ...
    tiny = (W == np.float32(1e-30)) & (D != 0)
    assert tiny.any() and (np.abs(m[1][tiny]) <= 1).all()                                        # ... the value stays a value
    assert (m[2][W == np.float32(3e38)] == np.float32(3e38)).all() and np.isfinite(m[1]).all()
    # under 3e38 a sample moves no stored value but a zero, which becomes F / 3e38: an fp32 subnormal
    heavy = W == np.float32(3e38)
    assert np.array_equal(bits(m[1][heavy & (D != 0)]), bits(D[heavy & (D != 0)]))
    assert (heavy & (D == 0)).any() and (np.abs(m[1][heavy & (D == 0)]) < np.float32(2.0 ** -126)).all() and (m[1][heavy & (D == 0)] != 0).any()


def test_caps_at_below_and_above_a_total():
    total, below, above, small = (np.float32(v) for v in S.CAPS)
    assert below < total < above and float(total) - float(below) == 2.0 ** -23 == float(above) - float(total)
    free = S.reference("weights", None)
    at = np.nonzero(free[2] == total)[0]
    assert len(at) > 0
    for cap in (total, below, above, small):
        m = S.reference("weights", float(cap))
        describe(("weights", float(cap)), m)
        assert np.array_equal(bits(m[1]), bits(free[1]))                                         # the cap moves no value
        assert np.array_equal(m[2], np.minimum(free[2], cap))
        assert (m[2][at] == min(total, cap)).all()
