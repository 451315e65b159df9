"""CPU suite: tests/tsdf_raycast_reference.py, the float64 twin of mi_tsdf_raycast, on cases with known answers: a hand-made slab whose values
are linear in x across a plane (the trilinear field is then exact), seen along an axis, obliquely, from behind and across a gap; the
fallback when a corner is unobserved; and the fused sphere, whose radius error is measured here and used by smoke()."""
import numpy as np

import tsdf_raycast_reference as RC
import tsdf_reference as R
from test_tsdf_reference import ORIGIN, sphere

ZERO = np.zeros(3, np.float32)
PLANE = 5.25


def at(t):
    T = np.eye(4)
    T[:3, 3] = t
    return T


def without(m, voxels):
    keep = ~(m[0][:, None, :] == np.array(voxels)[None, :, :]).all(axis=2).any(axis=1)
    return m[0][keep], m[1][keep], m[2][keep]


def test_a_slab_seen_along_an_axis_and_obliquely():
    m = RC.slab(PLANE, tau=4.0)            # values (5.25 - centre) / 4 on cx = 2 .. 7: 0.6875 .. -0.5625, exact in binary
    # along +x from x = 0.25: samples at 0.25 + k / 2; F(4.75) = 0.125 and F(5.25) = 0, so r = 1 and the depth is 5 exactly
    depth, xyz, nrm, hits, info = RC.raycast(m, ZERO, 1.0, 9.0, at([0.25, 4.3, 3.7]), [[2.0, 0, 0]], details=True)
    assert hits == 1 and info["trilinear"][0] == 1 and info["end_k"][0] == 10 and info["r"][0] == 1.0
    assert depth[0] == 5.0 and np.array_equal(xyz[0], np.array([5.25, 4.3, 3.7], np.float32)) and np.array_equal(nrm[0], [-1.0, 0.0, 0.0])
    # obliquely: the plane is met at t = (5.25 - o_x) / d_x; the field is linear, so only the roundings of d and of the depth remain: one fp32
    # spacing.  (The starts are chosen so that the first sample in the negative voxel layer, x >= 5, lies behind the plane: a sample with
    # 5 <= x < 5.25 ends the march with F still positive there, and r falls back to the voxels' values.)
    for start, direction, want in ((0.55, [4.0, 3.0, 0.0], 4.7 / 0.8), (0.3, [2.0, 1.0, 2.0], 4.95 * 1.5), (0.5, [1.0, 0.25, -0.125], 4.75 * np.sqrt(1 + 0.0625 + 0.015625))):
        depth, xyz, nrm, hits, info = RC.raycast(m, ZERO, 1.0, 12.0, at([start, 0.6, 1.2]), [direction], details=True)
        assert hits == 1 and info["trilinear"][0] == 1, direction
        assert abs(np.float64(depth[0]) - want) <= np.spacing(np.float32(want)) and abs(np.float64(xyz[0, 0]) - PLANE) <= np.spacing(np.float32(PLANE)), (direction, depth[0])
        assert np.array_equal(nrm[0], [-1.0, 0.0, 0.0])
    # the depth is along the unit direction whatever the length given, and min_range moves the samples, not the answer
    a = RC.raycast(m, ZERO, 1.0, 9.0, at([0.25, 4.3, 3.7]), [[1e-3, 0, 0], [7e5, 0, 0]])
    assert a[3] == 2 and a[0][0] == a[0][1] == 5.0
    b = RC.raycast(m, ZERO, 1.0, 9.0, at([0.25, 4.3, 3.7]), [[1.0, 0, 0]], min_range=2.125)
    assert b[3] == 1 and b[0][0] == 5.0


def test_misses():
    m = RC.slab(PLANE, tau=4.0)
    # from behind: the first observed sample is negative
    depth, xyz, nrm, hits, info = RC.raycast(m, ZERO, 1.0, 9.0, at([9.5, 4.5, 4.5]), [[-1.0, 0, 0]], details=True)
    assert hits == 0 and depth[0] == 0 and not xyz.any() and not nrm.any() and info["end_k"][0] == 4         # x = 7.5: the first sample in voxel 7
    # positive -> unobserved -> negative: the voxels of the last positive layer taken out along the ray
    gap = without(m, [[4, 4, 3]])
    depth, xyz, nrm, hits, info = RC.raycast(gap, ZERO, 1.0, 9.0, at([0.25, 4.3, 3.7]), [[1.0, 0, 0]], details=True)
    assert hits == 0 and info["end_k"][0] == 10 and depth[0] == 0
    # starting inside the negative side; no length; too short a range; past the map; the empty map
    assert RC.raycast(m, ZERO, 1.0, 9.0, at([6.5, 4.5, 4.5]), [[1.0, 0, 0]])[3] == 0
    assert RC.raycast(m, ZERO, 1.0, 9.0, at([0.25, 4.3, 3.7]), [[0.0, 0, 0]])[3] == 0
    assert RC.raycast(m, ZERO, 1.0, 4.75, at([0.25, 4.3, 3.7]), [[1.0, 0, 0]])[3] == 0
    assert RC.raycast(m, ZERO, 1.0, 5.0, at([0.25, 4.3, 3.7]), [[1.0, 0, 0]])[3] == 1                      # K = 11: sample 10 is the last
    assert RC.raycast(m, ZERO, 1.0, 9.0, at([0.25, 4.3, 30.0]), [[1.0, 0, 0]])[3] == 0
    assert RC.raycast(None, ZERO, 1.0, 9.0, None, [[1.0, 0, 0]])[3] == 0
    # a voxel below min_weight is unobserved
    light = (m[0], m[1], np.where((m[0] == [5, 4, 3]).all(axis=1), np.float32(0.5), m[2]))
    assert RC.raycast(light, ZERO, 1.0, 9.0, at([0.25, 4.3, 3.7]), [[1.0, 0, 0]])[3] == 0
    assert RC.raycast(light, ZERO, 1.0, 9.0, at([0.25, 4.3, 3.7]), [[1.0, 0, 0]], min_weight=0.5)[3] == 1


def test_the_fallback_when_a_corner_is_unobserved():
    # (5, 3, 4) is a corner of F at both ends and lies neither on the ray nor beside its two voxels: r falls back to the voxels' own values,
    # 0.1875 / (0.1875 + 0.0625) = 0.75, the depth to 4.5 + 0.75 / 2
    m = without(RC.slab(PLANE, tau=4.0), [[5, 3, 4]])
    depth, xyz, nrm, hits, info = RC.raycast(m, ZERO, 1.0, 9.0, at([0.25, 4.3, 3.7]), [[1.0, 0, 0]], details=True)
    assert hits == 1 and info["trilinear"][0] == 0 and info["r"][0] == 0.75 and depth[0] == 4.875 and xyz[0, 0] == 5.125
    assert np.array_equal(nrm[0], [-1.0, 0.0, 0.0])
    # on the low edge of the map the corners are missing altogether
    depth, xyz, nrm, hits, info = RC.raycast(RC.slab(PLANE, tau=4.0), ZERO, 1.0, 9.0, at([0.25, 0.3, 0.2]), [[1.0, 0, 0]], details=True)
    assert hits == 1 and info["trilinear"][0] == 0 and depth[0] == 4.875


def test_sphere_accuracy():
    """The sphere of test_tsdf_reference.py (radius 2, scanned from its centre along 4 000 directions, voxel 0.1, tau 0.3) cast from its centre
    along 2 000 random directions, range 4.  Measured over the seeds 0 .. 4: 901 .. 937 hits (4 000 rays leave holes in the band, and a ray
    that crosses a hole before the surface misses), largest |radius - 2| 0.0572 .. 0.0578, that is 0.58 voxel: where the trilinear field is
    not available r comes from two voxel values that were taken at the voxels' centres, not on the ray.  smoke() casts a map fused the same
    way; its bound is this number rounded up to one digit, 0.06."""
    m = R.integrate([sphere(4000)], None, ORIGIN, 0.1, 0.3)
    dirs = np.random.default_rng(100).normal(size=(2000, 3)).astype(np.float32)
    depth, xyz, nrm, hits, info = RC.raycast(m, ORIGIN, 0.1, 4.0, None, dirs, details=True)
    hit = depth > 0
    rad = np.linalg.norm(xyz[hit].astype(np.float64), axis=1)
    cos = (-xyz[hit].astype(np.float64) / rad[:, None] * nrm[hit]).sum(axis=1)
    print("sphere: %d hits of %d, %d by the trilinear field, radius error %.4f, median cos %.5f" % (hits, len(dirs), info["trilinear"].sum(), np.abs(rad - 2).max(), np.median(cos)))
    assert hits == hit.sum() > 800 and np.abs(rad - 2).max() <= 0.06 and np.median(cos) > 0.99
    assert np.abs(depth[hit] - rad).max() <= 5e-7                   # the sensor is at the centre: depth and radius are the same length
    assert not xyz[~hit].any() and not nrm[~hit].any()
    assert np.abs(np.linalg.norm(nrm[hit].astype(np.float64), axis=1) - 1).max() <= 2e-7
