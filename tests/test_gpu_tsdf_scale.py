"""GPU suite: mi_tsdf_integrate, mi_tsdf_extract and mi_tsdf_raycast on the cases of tests/tsdf_scale_cases.py, against tests/tsdf_reference.py
and tests/tsdf_raycast_reference.py bit for bit, through check and check_extract of tests/test_gpu_tsdf.py and check of
tests/test_gpu_tsdf_raycast.py, without a tolerance anywhere.  What the cases reach that the small scenes do not: the 20-bit sort of each
axis of the fusion (two radix passes, the result copied back from the input arrays), frames wider than 1024 voxels in the tables of the
extraction and the ray cast, the extents 1024, 1025 and 2^20 exactly, coordinates next to +-2^30, a thousand scans with runs of empty ones
under the rays' binary search, more than 256 tiles in the offsets scan, runs of ten thousand samples in one lane's sum, and stored weights
at which W + C rounds.  tests/test_tsdf_scale_cases.py shows on the CPU that every case is what it is named for."""
import numpy as np
import pytest

import tsdf_scale_cases as S
from test_gpu_tsdf import check, check_extract, raw_integrate
from test_gpu_tsdf_raycast import check as check_cast
from test_tsdf_reference import same_map

pytestmark = pytest.mark.gpu


def fused(ctx, capi, c, **over):
    """the case through mi_tsdf_integrate and the reference, bit for bit"""
    a = dict(scans=c["scans"], poses=c["poses"], map=c["map"])
    a.update(over)
    return check(ctx, capi, a["scans"], a["poses"], c["origin"], c["voxel"], c["tau"], map=a["map"], **c["kw"])


# ---- 1. fusion
@pytest.mark.parametrize("key", S.FUSION, ids=S.ident)
def test_fusion(ctx, capi, key):
    got = fused(ctx, capi, S.CASES[key[0]](*key[1:]))
    assert same_map(got, S.reference(*key)) and len(got[0]) > 0          # (the map tests/test_tsdf_scale_cases.py has described)


@pytest.mark.parametrize("axes", S.WIDE_AXES)
def test_wide_maps_scan_by_scan(ctx, capi, axes):
    # the stored map is itself wider than 1024 voxels from the third call on; the shells are apart, so the end is the map of the one call
    c = S.wide(axes)
    m = None
    for s, T in zip(c["scans"], c["poses"]):
        m = fused(ctx, capi, c, scans=[s], poses=[T], map=m)
    assert same_map(m, S.reference("wide", axes))


def test_the_capacity_protocol_on_a_wide_map(ctx, capi):
    c = S.wide("xz")
    want = S.reference("wide", "xz")
    xyz = np.concatenate(c["scans"])
    offsets = np.concatenate([[0], np.cumsum([len(s) for s in c["scans"]])])
    T = np.array(c["poses"]).transpose(0, 2, 1).astype(np.float32)
    params = capi.tsdf_params(voxel_size=c["voxel"], truncation=c["tau"])
    rc, nv, outs, _ = raw_integrate(ctx, capi, xyz, offsets, T, c["origin"], params, None, 0)                       # counts only
    assert rc == capi.MI_OK and nv == len(want[0])
    rc, nv, outs, _ = raw_integrate(ctx, capi, xyz, offsets, T, c["origin"], params, None, len(want[0]) - 1)        # one row short
    assert rc == capi.MI_OK and nv == len(want[0])
    assert (outs[0] == -7).all() and (outs[1] == -7).all() and (outs[2] == -7).all()
    rc, nv, outs, _ = raw_integrate(ctx, capi, xyz, offsets, T, c["origin"], params, None, len(want[0]))
    assert rc == capi.MI_OK and nv == len(want[0]) and same_map(outs, want)


# ---- 2. extraction
@pytest.mark.parametrize("key", S.SURFACES, ids=S.ident)
def test_extraction(ctx, capi, key):
    c, m = S.CASES[key[0]](*key[1:]), S.reference(*key)
    xyz, _ = check_extract(ctx, m, c["origin"], c["voxel"], min_weight=1.0)
    check_extract(ctx, m, c["origin"], c["voxel"], min_weight=2.0)
    if key[0] == "wide":                 # a point of every shell, so far apart: not two empty answers
        for T in c["poses"]:
            assert (np.linalg.norm(xyz.astype(np.float64) - T[:3, 3], axis=1) < 3.5).sum() > 100
    assert len(xyz) > 100


# ---- 3. ray casting, with empty-space skipping (where the driver finds it sound) and with every sample visited
@pytest.mark.parametrize("axes", S.WIDE_AXES)
def test_views_of_the_wide_maps(ctx, capi, axes):
    c, m = S.wide(axes), S.reference("wide", axes)
    inside, gap = S.inside_dirs("wide", axes), S.gap_length(axes)
    for T, dirs in zip(c["poses"], inside):
        assert check_cast(ctx, capi, m, c["origin"], c["voxel"], 5.0, T, dirs)[3] > 50
    dirs = np.concatenate([inside[0], S.gap_dirs(axes)])
    short = check_cast(ctx, capi, m, c["origin"], c["voxel"], gap - 10.0, c["poses"][0], dirs)
    assert short[3] > 50 and short[0].max() < 5.0            # below the gap: the first shell alone
    far = check_cast(ctx, capi, m, c["origin"], c["voxel"], gap + 10.0, c["poses"][0], dirs)
    assert far[3] > short[3] and (far[0][len(inside[0]):] > gap - 4.0).sum() >= 1       # above it: rays sent across hit the second shell
    assert np.array_equal(far[0][short[0] > 0], short[0][short[0] > 0])


@pytest.mark.parametrize("key", [k for k in S.SURFACES if k[0] != "wide"], ids=S.ident)
def test_views_of_the_edge_and_far_maps(ctx, capi, key):
    c, m = S.CASES[key[0]](*key[1:]), S.reference(*key)
    hits = 0
    for T, dirs in zip(c["poses"], S.inside_dirs(*key)):
        for max_range in (5.0, 60.0):    # 60: out of the occupied part, and in the far maps, whose samples collapse, as far as the next voxels
            hits += check_cast(ctx, capi, m, c["origin"], c["voxel"], max_range, T, dirs)[3]
    assert hits > 0
