"""mi_ndt_voxels and mi_ndt_system beyond the one small scene of tests/test_gpu_ndt.py: K27's scan and fix-up at the tile and wave edges
and over more tiles than the fix-up's wave has lanes, the voxel front's other sort paths and sizes, a cloud far from the origin, K28's
further workgroups, K30's table and its look-up (voxel_table.hpp: voxel_claim, voxel_row) on maps made by hand (a load of exactly one half, a probe chain past the last slot, an
extent of exactly 2^20 on every axis, coordinates down to -2^30 + 8, neighbours beyond either face of the listed box), K31's fold of up to
27 terms into all 28 sums, and positions voxel_axis refuses.  The cases and the proof that each is what it is named for:
tests/ndt_scale_cases.py, tests/test_ndt_scale_regimes.py.

No bound is new: the matrices go through check_voxels, the sums through assert_sums and check_system of tests/test_gpu_ndt.py -- every
row and every query, none skipped.  Every check prints the worst fraction of its bound it reached."""
import numpy as np
import pytest

import ndt_reference as N
import ndt_scale_cases as S
from test_gpu_ndt import assert_sums, bits, check_system, check_voxels, cube, scene, scene_map

pytestmark = pytest.mark.gpu


# ---- 1. K27 and its fix-up at the edges (both ratios: check_voxels' default)
def test_run_edges(ctx):
    cloud, lengths, named = S.run_edges()
    got = check_voxels(ctx, cloud, S.RUN_EDGES_VOXEL, S.RUN_EDGES_ORIGIN, "run edges")
    assert np.array_equal(got["count"], lengths) and got["count"].max() == 16384 + 300
    assert np.array_equal((got["icov"] != 0).any(axis=1), lengths >= 6)


# ---- 2. size, sort paths and offset
@pytest.mark.parametrize("n,shifted", [(S.SORT_ONE_PASS + 1, False), (70001, False), (70001, True)])
def test_uniform_clouds(ctx, n, shifted):
    cloud, voxel, origin = S.uniform_case(n, shifted)
    got = check_voxels(ctx, cloud, voxel, origin, "uniform %d%s" % (n, " shifted" if shifted else ""))
    assert len(got["count"]) > 256 and int(got["count"].sum()) == n


@pytest.mark.parametrize("which", range(len(S.SORT_PATH_EXTENTS)))
def test_sort_path_clouds(ctx, which):
    for turn in range(3):
        cloud, voxel, origin, extents = S.sort_path_case(which, turn)
        got = check_voxels(ctx, cloud, voxel, origin, "extents %s" % (extents,))
        assert len(got["count"]) > 256 and int(got["count"].sum()) == len(cloud)


# ---- 3. the table and the lookup on maps made by hand
def check_lookup(ctx, queries, vox, ref, nb, what):
    sums, centre, idx, terms = ctx.ndt_system(queries, vox, None, nb)
    assert np.array_equal(idx, ref["idx"]), (what, np.flatnonzero(idx != ref["idx"])[:8])
    assert np.array_equal(terms, ref["terms"]), (what, np.flatnonzero(terms != ref["terms"])[:8])
    assert np.array_equal(bits(centre), bits(ref["centre"])), what
    assert_sums(sums, ref, len(queries), what)
    return sums, centre, idx, terms


@pytest.mark.parametrize("nb", S.NEIGHBOURHOODS)
@pytest.mark.parametrize("name", S.MAP_CASES)
def test_maps_made_by_hand(ctx, name, nb):
    vox, queries = S.map_case(name)
    check_lookup(ctx, queries, vox, S.map_reference(name, nb), nb, "%s neighbourhood %d" % (name, nb))


def test_all_sums_on_the_cube(ctx):
    """test_gpu_ndt.py::test_lookup_against_the_dictionary's maps and queries with all of sums[:28] held to the restatement: the fold of up
    to 27 terms per point on a map of 2 000 voxels.  The matrices are the device's own (they are checked in the tests above)."""
    cloud, queries = cube()
    vox = ctx.ndt_voxels(cloud, 0.8, (0.3, 0.1, -0.2), 3, 0.01)
    holes = dict(vox, icov=vox["icov"].copy())
    holes["icov"][::5] = 0
    for label, m in (("full", vox), ("holes", holes), ("one row", {k: (v[700:701] if k in ("coord", "mean", "icov", "count") else v) for k, v in vox.items()})):
        lookup = N.Lookup(m)
        for nb in S.NEIGHBOURHOODS:
            ref = N.sums_at(queries, m, nb, lookup=lookup)
            sums, _, _, terms = check_lookup(ctx, queries, m, ref, nb, "cube %s neighbourhood %d" % (label, nb))
            assert label != "full" or (sums[28] > 2500 and (nb == 1 or terms.max() > nb // 2))


# ---- 4. positions voxel_axis refuses
@pytest.mark.parametrize("nb", S.NEIGHBOURHOODS)
def test_refused_positions(ctx, nb):
    vox = scene_map(ctx, "origin")
    cloud, T, out = S.refused_case(scene("origin")[0], vox)
    sums, centre, idx, terms = check_system(ctx, cloud, vox, T, nb, "refused positions neighbourhood %d" % nb)
    assert (idx[out] == -1).all() and (terms[out] == 0).all()
    rest = np.setdiff1d(np.arange(len(cloud)), out)
    assert (idx[rest] >= 0).sum() > 1500 and sums[28] > 1500 and (terms[rest] > 0).sum() == sums[28]
