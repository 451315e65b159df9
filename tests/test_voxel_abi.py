"""CPU suite: the voxel entry points exist, mi_voxel_index (a pure host function) is the float32 expression the header states, and
the float64 restatement the GPU tests use as their oracle (tests/voxel_reference.py) is right on clouds worked by hand."""
import ctypes as C

import numpy as np
import pytest

import voxel_reference as V


def test_library_exports_the_voxel_entry_points(capi):
    lib = capi.lib()
    for name in ("mi_voxel_index", "mi_voxel_downsample"):
        assert hasattr(lib, name), name
        assert name in capi.EXPORTS, name
    assert lib.mi_abi_version() == 4          # additive: no signature of version 4 changed


def index_all(capi, pts, origin, voxel):
    """mi_voxel_index on every row of pts -> int32 [n, 3] (raw calls: no array is built per point)."""
    pts = np.ascontiguousarray(pts, np.float32)
    origin = np.ascontiguousarray(origin, np.float32)
    out = np.full((len(pts), 3), -12345, np.int32)
    for i in range(len(pts)):
        rc = capi.voxel_index_raw(pts.ctypes.data + 12 * i, origin.ctypes.data, float(voxel), out.ctypes.data + 12 * i)
        assert rc == capi.MI_OK, (i, capi.lib().mi_last_error())
    return out


@pytest.mark.parametrize("voxel", [0.1, 0.25, 1.0 / 3.0, 7.0])
def test_voxel_index_is_the_float32_expression_on_random_points(capi, voxel):
    rng = np.random.default_rng(11)
    pts = rng.uniform(-50.0, 50.0, (10 ** 4, 3)).astype(np.float32)
    origin = np.array([-3.25, 0.7, 12.125], np.float32)
    got = index_all(capi, pts, origin, voxel)
    assert np.array_equal(got, V.voxel_coords(pts, voxel, origin))
    assert np.array_equal(capi.voxel_index(pts[5], origin, voxel), got[5])


@pytest.mark.parametrize("voxel", [0.1, 0.25, 1.0 / 3.0, 7.0])
def test_voxel_index_on_lattice_points_where_the_division_rounding_decides(capi, voxel):
    # p = o + fl32(k v): the quotient (p - o) / v lies within an ulp of the integer k, so the voxel is k or k - 1 by the rounding of the
    # one subtraction and the one division -- a reciprocal multiply or a fused step would land on the other side for some k
    v = np.float32(voxel)
    k = np.arange(-50, 51).astype(np.float32)
    for origin in (np.zeros(3, np.float32), np.array([0.3, -1.7, 1000.1], np.float32)):
        pts = (origin[None, :] + (k * v)[:, None]).astype(np.float32)
        got = index_all(capi, pts, origin, voxel)
        want = V.voxel_coords(pts, voxel, origin)
        assert np.array_equal(got, want)
        assert np.abs(want - np.arange(-50, 51)[:, None]).max() <= 1


def test_voxel_index_argument_errors(capi):
    p, o = np.array([1, 2, 3], np.float32), np.zeros(3, np.float32)
    for voxel in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(capi.MiSlamError):
            capi.voxel_index(p, o, voxel)
    with pytest.raises(capi.MiSlamError):
        capi.voxel_index(np.array([1, np.nan, 3], np.float32), o, 1.0)
    with pytest.raises(capi.MiSlamError):
        capi.voxel_index(p, np.array([np.inf, 0, 0], np.float32), 1.0)
    # the quotient's range is [-2^30, 2^30): 2^30 itself is refused, the largest float below it and -2^30 are voxels
    edge = np.float32(2.0 ** 30)
    with pytest.raises(capi.MiSlamError) as e:
        capi.voxel_index(np.array([edge, 0, 0], np.float32), o, 1.0)
    assert "2^30" in str(e.value)
    with pytest.raises(capi.MiSlamError):
        capi.voxel_index(np.array([0, 0, 1e12], np.float32), o, 1.0)
    with pytest.raises(capi.MiSlamError):
        capi.voxel_index(np.array([0, -np.nextafter(edge, np.float32(np.inf)), 0], np.float32), o, 1.0)
    assert capi.voxel_index(np.array([np.nextafter(edge, np.float32(0)), -edge, 0], np.float32), o, 1.0).tolist() == [2 ** 30 - 64, -2 ** 30, 0]
    # a refused call leaves `out` as it was
    out = np.full(3, 77, np.int32)
    rc = capi.voxel_index_raw(p.ctypes.data, o.ctypes.data, 0.0, out.ctypes.data)
    assert rc == capi.MI_ERR_INVALID_ARG and out.tolist() == [77, 77, 77]
    assert capi.voxel_index_raw(None, o.ctypes.data, 1.0, out.ctypes.data) == capi.MI_ERR_INVALID_ARG


def test_reference_on_a_cloud_worked_by_hand():
    # voxel 1, origin = the minimum (0, 0, 0); voxels: (0,0,0) x 2, (1,0,0), (0,1,0), (0,0,1) x 2 -> rows ascending by (cz, cy, cx)
    pts = np.array([[0.25, 0.5, 0.0], [1.5, 0.25, 0.5], [0.0, 0.0, 1.5], [0.75, 0.0, 0.5], [0.5, 1.0, 0.25], [0.5, 0.5, 1.0]], np.float32)
    cen, cnt, coord, vmap = V.downsample(pts, 1.0)
    assert coord.tolist() == [[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]]
    assert cnt.tolist() == [2, 1, 1, 2] and vmap.tolist() == [0, 1, 3, 0, 2, 3]
    assert cen.tolist() == [[0.5, 0.25, 0.25], [1.5, 0.25, 0.5], [0.5, 1.0, 0.25], [0.25, 0.25, 1.25]]
    assert cen.dtype == np.float32 and cnt.dtype == np.int32 and coord.dtype == np.int32 and vmap.dtype == np.int32


def test_reference_with_negative_coordinates_under_an_explicit_origin():
    # origin (0, 0, 0), voxel 2: floor division sends -0.5 to voxel -1 and -2 to voxel -1 as well, -2.5 to -2
    pts = np.array([[-0.5, 0.5, 0.0], [3.0, -2.0, 1.0], [-2.5, 1.0, -0.25], [-1.0, 1.5, 1.5], [2.5, -0.5, 0.5]], np.float32)
    cen, cnt, coord, vmap = V.downsample(pts, 2.0, origin=[0, 0, 0])
    assert coord.tolist() == [[-2, 0, -1], [1, -1, 0], [-1, 0, 0]]
    assert cnt.tolist() == [1, 2, 2] and vmap.tolist() == [2, 1, 0, 2, 1]
    assert cen.tolist() == [[-2.5, 1.0, -0.25], [2.75, -1.25, 0.75], [-0.75, 1.0, 0.75]]


def test_reference_single_voxel_and_one_voxel_per_point():
    pts = np.array([[1.0, 2.0, 3.0], [2.0, 4.0, 5.0], [3.0, 3.0, 4.0]], np.float32)
    cen, cnt, coord, vmap = V.downsample(pts, 100.0)
    assert coord.tolist() == [[0, 0, 0]] and cnt.tolist() == [3] and vmap.tolist() == [0, 0, 0] and cen.tolist() == [[2.0, 3.0, 4.0]]
    cen, cnt, coord, vmap = V.downsample(pts, 0.5)           # origin (1, 2, 3): voxels (0,0,0), (2,4,4), (4,2,2)
    assert coord.tolist() == [[0, 0, 0], [4, 2, 2], [2, 4, 4]] and cnt.tolist() == [1, 1, 1] and vmap.tolist() == [0, 2, 1]
    assert np.array_equal(cen, pts[[0, 2, 1]])
