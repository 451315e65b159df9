"""CPU suite: the restatement of mi_radius_search (tests/radius_reference.py) against facts worked by hand on the 3 x 3 x 3 integer lattice
of tests/test_knn_abi.py: the centre's ball at four radii, a point exactly at r2, self mode by index, an empty row's offset."""
import numpy as np
import pytest

import knn_reference as K
import radius_reference as R
from test_knn_abi import lattice3

MODES = (K.DIST_CPU_ROUNDING, K.DIST_FMA)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("r2,members", [(0.5, 1), (1.0, 7), (2.0, 19), (3.0, 27)])
def test_the_centre_of_the_lattice_has_the_hand_counted_ball(mode, r2, members):
    L = lattice3()
    radius = np.sqrt(np.float32(r2))                   # the float32 root, or its upper neighbour where the root's square rounds below r2
    if R.r2_of(radius) < np.float32(r2):
        radius = np.nextafter(radius, np.float32(np.inf))
    assert np.float32(r2) <= R.r2_of(radius) < np.float32(r2) + np.float32(1e-6)
    offsets, idx, d2, total = R.search(np.array([[1, 1, 1]], np.float32), L, radius, mode)
    assert total == members and offsets.tolist() == [0, members] and offsets.dtype == np.int64
    # the centre itself, the six faces at 1, the twelve edges at 2, the eight corners at 3, each group in index order
    faces, edges = [4, 10, 12, 14, 16, 22], [1, 3, 5, 7, 9, 11, 15, 17, 19, 21, 23, 25]
    corners = [0, 2, 6, 8, 18, 20, 24, 26]
    want = ([13] + faces + edges + corners)[:members]
    assert idx.tolist() == want and d2.tolist() == ([0.0] + [1.0] * 6 + [2.0] * 12 + [3.0] * 8)[:members]


@pytest.mark.parametrize("mode", MODES)
def test_a_point_exactly_at_r2_belongs_and_one_ulp_beyond_does_not(mode):
    cloud = np.array([[0, 0, 0], [3, 0, 0], [0, 4, 0], [3, 4, 0]], np.float32)
    q = np.zeros((1, 3), np.float32)
    assert R.search(q, cloud, 5.0, mode)[1].tolist() == [0, 1, 2, 3]                  # |(3, 4, 0)|^2 = 25 = r2 exactly
    assert R.search(q, cloud, np.nextafter(np.float32(5.0), np.float32(0)), mode)[1].tolist() == [0, 1, 2]
    assert R.search(q, cloud, 4.0, mode)[1].tolist() == [0, 1, 2] and R.search(q, cloud, 3.0, mode)[1].tolist() == [0, 1]


@pytest.mark.parametrize("mode", MODES)
def test_self_mode_drops_by_index_and_keeps_a_duplicate_at_zero(mode):
    cloud = np.array([[0, 0, 0], [1, 0, 0], [0, 0, 0], [9, 9, 9]], np.float32)       # point 2 duplicates point 0
    offsets, idx, d2, total = R.search(None, cloud, 1.0, mode)
    assert offsets.tolist() == [0, 2, 4, 6, 6] and total == 6
    assert idx.tolist() == [2, 1, 0, 2, 0, 1] and d2.tolist() == [0.0, 1.0, 1.0, 1.0, 0.0, 1.0]
    assert np.signbit(d2).sum() == 0                                                    # the duplicate is at +0
    # the same points as a separate query set: nothing is dropped, every point finds itself
    offsets_q, idx_q, _, total_q = R.search(cloud, cloud, 1.0, mode)
    assert offsets_q.tolist() == [0, 3, 6, 9, 10] and total_q == 10 and idx_q.tolist() == [0, 2, 1, 1, 0, 2, 0, 2, 1, 3]


def test_an_empty_row_leaves_its_offset_unchanged():
    L = lattice3()
    q = np.array([[1, 1, 1], [50, 50, 50], [0, 0, 0], [-50, 0, 0]], np.float32)
    offsets, idx, _, total = R.search(q, L, 1.0)
    assert offsets.tolist() == [0, 7, 7, 11, 11] and total == 11 and idx[7:].tolist() == [0, 1, 3, 9]
    offsets0, keys0, total0 = R.csr(R.rows(q[[1, 3]], L, 1.0))
    assert offsets0.tolist() == [0, 0, 0] and total0 == 0 and keys0.shape == (0,) and keys0.dtype == np.uint64


def test_pack_and_unpack_are_inverse():
    keys = np.concatenate(R.rows(None, lattice3(), 1.5))
    idx, d2 = R.unpack(keys)
    assert idx.dtype == np.int32 and d2.dtype == np.float32 and np.array_equal(R.pack(idx, d2), keys)
