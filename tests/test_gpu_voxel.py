"""GPU suite: mi_voxel_downsample against the float64 restatement of tests/voxel_reference.py.

Structure (row count, voxel coordinates, counts, the point -> row map) is compared exactly.  Centroids are compared bit for bit on
clouds quantised to multiples of 2^-10 inside +-512 -- there every fp64 partial sum is exact in any order, so the value is determined
-- and to one fp32 ulp on raw fp32 clouds: an fp64 sum of n fp32 terms is off by at most n 2^-53 relative to sum |x|, which can move
the fp32 rounding only at a tie."""
import ctypes as C
import functools

import numpy as np
import pytest

import voxel_reference as V

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 1000, 5000]
VOXELS = [0.1, 1.0, 20.0]
BELOW = np.array([-10.0, -10.0, -10.0], np.float32)      # with voxel 20 every point of [-5, 5]^3 falls into voxel (0, 0, 0)


def quantise(p):
    return (np.round(np.asarray(p, np.float64) * 1024.0) / 1024.0).astype(np.float32)


@functools.lru_cache(maxsize=None)
def cloud(n, quantised, seed=5):
    p = np.random.default_rng(seed + n).uniform(-5.0, 5.0, (n, 3)).astype(np.float32)
    p = quantise(p) if quantised else p
    p.setflags(write=False)
    return p


def origin_for(voxel):
    return BELOW if voxel == 20.0 else None


@functools.lru_cache(maxsize=None)
def reference(n, quantised, voxel):
    return V.downsample(cloud(n, quantised), voxel, origin_for(voxel))


def device(ctx, pts, voxel, origin):
    return ctx.voxel_downsample(pts, voxel, origin, want_counts=True, want_coords=True, want_map=True)


def assert_structure(got, ref):
    (cen, cnt, coord, vmap), (rcen, rcnt, rcoord, rvmap) = got, ref
    assert len(cen) == len(rcen) == len(cnt) == len(coord)
    assert np.array_equal(coord, rcoord)
    assert np.array_equal(cnt, rcnt) and int(cnt.sum()) == len(vmap)
    assert np.array_equal(vmap, rvmap)


def assert_bitwise(got, ref):
    assert np.array_equal(got[0].view(np.uint32), ref[0].view(np.uint32))


def assert_one_ulp(got, ref):
    g, r = got[0].astype(np.float64), ref[0].astype(np.float64)
    ulp = np.maximum(np.spacing(np.abs(ref[0])), np.spacing(np.abs(got[0]))).astype(np.float64)
    worst = float(np.max(np.abs(g - r) / ulp)) if len(g) else 0.0
    assert worst <= 1.0, worst


def assert_matches_voxel_index(capi, pts, voxel, origin, got):
    """the row a point is mapped to carries the voxel mi_voxel_index gives for the point"""
    pts = np.ascontiguousarray(pts, np.float32)
    o = np.ascontiguousarray(pts.min(axis=0) if origin is None else origin, np.float32)
    idx = np.empty((len(pts), 3), np.int32)
    for i in range(len(pts)):
        assert capi.voxel_index_raw(pts.ctypes.data + 12 * i, o.ctypes.data, float(voxel), idx.ctypes.data + 12 * i) == capi.MI_OK
    assert np.array_equal(got[2][got[3]], idx)


def check_all(ctx, capi, raw, voxel, origin):
    """rows 1-3 of the plan on one cloud: structure + mi_voxel_index + one ulp on the raw cloud, structure + bits on the quantised one"""
    ref = V.downsample(raw, voxel, origin)
    got = device(ctx, raw, voxel, origin)
    assert_structure(got, ref)
    assert_matches_voxel_index(capi, raw, voxel, origin, got)
    assert_one_ulp(got, ref)
    q = quantise(raw)
    refq, gotq = V.downsample(q, voxel, origin), device(ctx, q, voxel, origin)
    assert_structure(gotq, refq)
    assert_bitwise(gotq, refq)
    return got, gotq


@pytest.mark.parametrize("voxel", VOXELS)
@pytest.mark.parametrize("n", SIZES)
def test_structure_is_exact(ctx, capi, n, voxel):
    pts, origin = cloud(n, False), origin_for(voxel)
    got, ref = device(ctx, pts, voxel, origin), reference(n, False, voxel)
    assert_structure(got, ref)
    assert_matches_voxel_index(capi, pts, voxel, origin, got)
    if voxel == 20.0:
        assert len(got[0]) == 1 and got[2].tolist() == [[0, 0, 0]]        # everything in one voxel
    if voxel == 0.1:
        assert len(got[0]) >= 0.99 * n                                      # almost every point its own voxel
    # the optional outputs are optional: the centroids alone are the same bits
    assert np.array_equal(ctx.voxel_downsample(pts, voxel, origin).view(np.uint32), got[0].view(np.uint32))


@pytest.mark.parametrize("voxel", VOXELS)
@pytest.mark.parametrize("n", SIZES)
def test_centroids_bitwise_on_quantised_clouds(ctx, n, voxel):
    got, ref = device(ctx, cloud(n, True), voxel, origin_for(voxel)), reference(n, True, voxel)
    assert_structure(got, ref)
    assert_bitwise(got, ref)


@pytest.mark.parametrize("voxel", VOXELS)
@pytest.mark.parametrize("n", SIZES)
def test_centroids_within_one_ulp_on_raw_clouds(ctx, n, voxel):
    got, ref = device(ctx, cloud(n, False), voxel, origin_for(voxel)), reference(n, False, voxel)
    assert_one_ulp(got, ref)


def test_long_run_in_the_middle_of_the_sorted_order(ctx, capi):
    # 3000 points in ONE voxel (12, 12, 12 of the lattice at origin -6, voxel 0.5: z ~ 0, the middle of the (cz, cy, cx) order) between
    # 5000 spread out: a run that spans 47 waves and 12 workgroups of the segmented sum, with short runs on both sides
    rng = np.random.default_rng(21)
    dense = rng.uniform(0.05, 0.45, (3000, 3)).astype(np.float32)
    spread = rng.uniform(-5.0, 5.0, (5000, 3)).astype(np.float32)
    pts = np.concatenate([spread[:2500], dense, spread[2500:]])[rng.permutation(8000)]
    got, gotq = check_all(ctx, capi, pts, 0.5, np.array([-6, -6, -6], np.float32))
    row = int(np.argmax(got[1]))
    assert got[1][row] >= 3000 and got[2][row].tolist() == [12, 12, 12]
    assert 0.25 * len(got[0]) < row < 0.75 * len(got[0])


def test_long_run_that_is_the_whole_cloud(ctx, capi):
    got, gotq = check_all(ctx, capi, cloud(5000, False), 20.0, BELOW)
    assert got[1].tolist() == [5000] and gotq[1].tolist() == [5000]


def lattice_cloud(rng, n, extents, ends_axis):
    """n points of the lattice at origin 0, voxel 1, spread over `extents` voxels per axis; two of them pin the extent of
    `ends_axis` to exactly extents[ends_axis].  Coordinates reach 2^20 here, beyond the +-512 of the other quantised clouds, and stay
    multiples of 2^-10 (of 2^-4 near 2^20): at most 30 significant bits each and at most 3000 terms, so every fp64 sum is still exact."""
    p = np.stack([rng.uniform(0.0, e - max(0.01, e * 2.0 ** -22), n) for e in extents], axis=1)     # (the margin: rounding to fp32 and to 2^-10 must not reach e itself)
    p[0, ends_axis], p[1, ends_axis] = 0.5, extents[ends_axis] - 0.5
    p = quantise(p)
    c = V.voxel_coords(p, 1.0, np.zeros(3))
    assert (c.max(axis=0) - c.min(axis=0) + 1).tolist()[ends_axis] == extents[ends_axis]
    return p


@pytest.mark.parametrize("extents", [(1024, 1024, 1024), (1025, 1024, 1024), (5, 2000, 70000), (2 ** 20, 30, 30)])
def test_every_sort_path(ctx, capi, extents):
    # all extents <= 1024: one packed 30-bit key; one extent of 1025: a stable sort per axis; extents that need two radix digits; the limit
    rng = np.random.default_rng(31)
    for axis in range(3):
        pts = lattice_cloud(rng, 3000, extents, int(np.argmax(extents)))
        got, ref = device(ctx, pts, 1.0, np.zeros(3, np.float32)), V.downsample(pts, 1.0, np.zeros(3))
        assert_structure(got, ref)
        assert_bitwise(got, ref)
        extents = extents[1:] + extents[:1]           # the same extents on the other axes
    assert_matches_voxel_index(capi, pts, 1.0, np.zeros(3, np.float32), got)


def test_extent_limit(ctx, capi):
    rng = np.random.default_rng(32)
    ok = lattice_cloud(rng, 500, (2 ** 20, 8, 8), 0)
    assert len(ctx.voxel_downsample(ok, 1.0, np.zeros(3, np.float32))) > 400
    too_wide = ok.copy()
    too_wide[1, 0] = 2.0 ** 20 + 0.5                   # voxels 0 .. 2^20: an extent of 2^20 + 1
    with pytest.raises(capi.MiSlamError) as e:
        ctx.voxel_downsample(too_wide, 1.0, np.zeros(3, np.float32))
    assert "libmislam error %d" % capi.MI_ERR_INVALID_ARG in str(e.value) and "axis 0" in str(e.value)
    assert len(ctx.voxel_downsample(too_wide, 2.0, np.zeros(3, np.float32))) > 100       # a larger voxel fits


def test_radix_chunk_edge(ctx, capi):
    # 4096 * 64 + 1 points: the sort's chunks stop being single 64-element steps; voxel 0.25 over [-5, 5]^3: about 4 points per voxel
    n = 4096 * 64 + 1
    pts = cloud(n, True)
    got, ref = device(ctx, pts, 0.25, None), V.downsample(pts, 0.25)
    assert 3.5 < n / len(ref[0]) < 4.5
    assert_structure(got, ref)
    assert_matches_voxel_index(capi, pts, 0.25, None, got)
    assert_bitwise(got, ref)


def test_order_independence(ctx):
    pts = cloud(5000, True)
    rng = np.random.default_rng(41)
    a = device(ctx, pts[rng.permutation(5000)], 0.5, None)
    b = device(ctx, pts[rng.permutation(5000)], 0.5, None)
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[1], b[1])
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
    raw = cloud(5000, False)                           # raw fp32: the structure does not depend on the order either
    a, b = device(ctx, raw[rng.permutation(5000)], 0.5, None), device(ctx, raw[rng.permutation(5000)], 0.5, None)
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[1], b[1])


def test_determinism_and_isolation(ctx, capi, golden):
    def same(a, b):
        return all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))

    pts = cloud(5000, False)
    first = device(ctx, pts, 0.5, None)
    assert same(device(ctx, pts, 0.5, None), first)
    z = golden.npz("synth2k_clouds.npz")
    params = capi.icp_params(max_iterations=8)
    ctx.icp_register(z["before"], z["after"], params)
    assert same(device(ctx, pts, 0.5, None), first)
    # a loaded ICP problem survives a downsample call between its load and its run
    ctx.icp_load(z["before"], z["after"], params)
    ctx.icp_run(8)
    R0, t0, it0, err0, why0 = ctx.icp_result()
    ctx.icp_load(z["before"], z["after"], params)
    assert same(device(ctx, pts, 0.5, None), first)
    ctx.icp_run(8)
    R1, t1, it1, err1, why1 = ctx.icp_result()
    assert it0 > 0 and (it1, why1) == (it0, why0)
    assert np.array_equal(R1.view(np.uint32), R0.view(np.uint32)) and np.array_equal(t1.view(np.uint32), t0.view(np.uint32))
    assert np.float32(err1).tobytes() == np.float32(err0).tobytes()


def raw_call(ctx, capi, pts, n, voxel, origin=None):
    """mi_voxel_downsample with every output prefilled with a sentinel -> (error code, message, outputs untouched?)"""
    pts = np.ascontiguousarray(pts, np.float32)
    cap = max(len(pts), 1)
    out = np.full((cap, 3), -7.5, np.float32)
    cnt, coord, vmap = np.full(cap, -7, np.int32), np.full((cap, 3), -7, np.int32), np.full(cap, -7, np.int32)
    rows = C.c_int(-7)
    rc = capi.voxel_downsample_raw(ctx._h, pts.ctypes.data, n, float(voxel), None if origin is None else origin.ctypes.data,
                                   out.ctypes.data, C.addressof(rows), cnt.ctypes.data, coord.ctypes.data, vmap.ctypes.data)
    untouched = bool((out == -7.5).all() and (cnt == -7).all() and (coord == -7).all() and (vmap == -7).all() and rows.value == -7)
    return rc, capi.lib().mi_last_error().decode(), untouched


def test_errors_leave_the_outputs_untouched(ctx, capi):
    good = cloud(1000, False)
    bad = good.copy()
    bad[17, 1] = np.nan
    bad[400, 0] = np.inf                               # the LOWEST offending index is the one reported
    rc, msg, untouched = raw_call(ctx, capi, bad, 1000, 0.5)
    assert rc == capi.MI_ERR_INVALID_ARG and untouched and "point 17 " in msg
    with pytest.raises(capi.MiSlamError) as e:
        ctx.voxel_downsample(bad, 0.5)
    assert "17" in str(e.value)
    rc, msg, untouched = raw_call(ctx, capi, good, 0, 0.5)
    assert rc == capi.MI_ERR_INVALID_ARG and untouched
    for voxel in (0.0, -1.0, float("nan"), float("inf")):
        rc, msg, untouched = raw_call(ctx, capi, good, 1000, voxel)
        assert rc == capi.MI_ERR_INVALID_ARG and untouched and "voxel_size" in msg
    rc, msg, untouched = raw_call(ctx, capi, good, 1000, 1e-6)       # NULL origin, [-5, 5] / 1e-6: 1e7 voxels per axis
    assert rc == capi.MI_ERR_INVALID_ARG and untouched and "2^20" in msg
    far = good.copy()
    far[33, 2] = 3.0e9                                  # (3e9 + 10) / 1 > 2^30
    rc, msg, untouched = raw_call(ctx, capi, far, 1000, 1.0, BELOW)
    assert rc == capi.MI_ERR_INVALID_ARG and untouched and "point 33:" in msg
    out, rows = np.empty((1000, 3), np.float32), C.c_int(0)
    assert capi.voxel_downsample_raw(ctx._h, None, 1000, 0.5, None, out.ctypes.data, C.addressof(rows), None, None, None) == capi.MI_ERR_INVALID_ARG
    assert capi.voxel_downsample_raw(ctx._h, good.ctypes.data, 1000, 0.5, None, None, C.addressof(rows), None, None, None) == capi.MI_ERR_INVALID_ARG
    assert capi.voxel_downsample_raw(ctx._h, good.ctypes.data, 1000, 0.5, None, out.ctypes.data, None, None, None, None) == capi.MI_ERR_INVALID_ARG
    assert len(ctx.voxel_downsample(good, 0.5)) > 0     # and the context still works
