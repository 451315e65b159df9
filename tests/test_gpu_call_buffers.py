"""GPU suite: what the drivers' buffer list (cuda-slam_amd/csrc/call_buffers.hpp) must keep -- a context whose buffers have grown, shrunk and
been skipped answers exactly as a new one.  Every point-cloud call runs on one context at n = 300, 5, 70, 1000, 70 (growth, below one
wave, across 64 and the 256-point scan tile, beyond the first allocation's one-and-a-half rule, and back), first with every optional output
asked for, then with none, then once more with all of them at n = 1000; every returned array and count is compared for exact equality with
what a new context returns for the same input and the same outputs.  Output arrays start as zeros, so what a call leaves unwritten compares too.

Every call keeps its buffers in a struct of its own in the context, so one new context is new to each call made on it once; the second
variant of a call (separate queries, the radius method, the counted clustering) takes a second one.  Seeded uniform clouds in the unit cube;
k = 4, a radius of 0.5 and min_neighbours 1, so that five points are enough for every call."""
import ctypes as C
import functools

import numpy as np
import pytest

import ndt_reference as NR
from conftest import load_package

SIZES = (300, 5, 70, 1000, 70)
K, RADIUS = 4, 0.5
NDT_VOXEL, NDT_MIN_POINTS = 0.75, 3      # the voxel at the cloud's lower corner takes 0.75^3 of the cube: five points leave three in it (checked below)


def cloud(n, seed):
    return np.random.default_rng(1000 * seed + n).uniform(0, 1, (n, 3)).astype(np.float32)


def unit(n, seed):
    v = np.random.default_rng(1000 * seed + n).normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def cov6(n, seed):
    a = np.random.default_rng(1000 * seed + n).uniform(-1, 1, (n, 3, 3))
    m = 0.01 * (a @ a.transpose(0, 2, 1) + 0.1 * np.eye(3))
    return np.stack([m[:, i, j] for i, j in NR.TRI], axis=1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def ndt_map():
    """a voxel map of a 500-point cloud by the numpy restatement: the fixed side of ndt_system"""
    v = NR.voxels(cloud(500, 11), 0.25, min_points=NDT_MIN_POINTS)
    return {k: v[k] for k in ("coord", "mean", "icov", "origin", "voxel")}


def ptr(a, wanted=True):
    return a.ctypes.data if wanted else None


def as_tuple(r):
    return r if isinstance(r, tuple) else (r,)


# ---- the calls: (capi, ctx, n, full) -> a tuple of arrays and numbers
def knn_self(capi, ctx, n, full):
    return as_tuple(ctx.knn_search(None, cloud(n, 1), K, want_d2=full, want_count=full))


def knn_queries(capi, ctx, n, full):
    return as_tuple(ctx.knn_search(cloud(n, 2), cloud(n, 1), K, want_d2=full, want_count=full))


def normals(capi, ctx, n, full):
    return as_tuple(ctx.estimate_normals(cloud(n, 1), K, want_curvature=full, want_count=full))


def covariances(capi, ctx, n, full):
    return as_tuple(ctx.estimate_covariances(cloud(n, 1), K, want_count=full))


def outliers(method):
    def call(capi, ctx, n, full):
        xyz, p = cloud(n, 3), capi.outlier_params(method=method, k=K, radius=RADIUS, min_neighbours=1)
        statistical = method == capi.OUTLIER_STATISTICAL
        out_xyz, out_index, kept = np.zeros((n, 3), np.float32), np.zeros(n, np.int32), C.c_int(-1)
        keep, mean, neighbours, stats = np.zeros(n, np.uint8), np.zeros(n, np.float32), np.zeros(n, np.int32), capi.OutlierStats()
        capi._check(capi.remove_outliers_raw(ctx._h, xyz.ctypes.data, n, C.addressof(p), ptr(out_xyz, full), ptr(out_index, full), C.addressof(kept),
                                             ptr(keep, full), ptr(mean, full and statistical), ptr(neighbours, full), C.addressof(stats) if full else None))
        return out_xyz, out_index, kept.value, keep, mean, neighbours, stats.mean, stats.stddev, stats.threshold, stats.kept
    return call


def iss(capi, ctx, n, full):
    xyz, p = cloud(n, 4), capi.iss_params(salient_radius=RADIUS, non_max_radius=RADIUS, min_neighbours=1)
    out_xyz, out_index, kept = np.zeros((n, 3), np.float32), np.zeros(n, np.int32), C.c_int(-1)
    flag, saliency, eig, neighbours = np.zeros(n, np.uint8), np.zeros(n, np.float32), np.zeros((n, 3), np.float32), np.zeros(n, np.int32)
    capi._check(capi.iss_keypoints_raw(ctx._h, xyz.ctypes.data, n, C.addressof(p), ptr(out_xyz, full), ptr(out_index, full), C.addressof(kept),
                                       ptr(flag, full), ptr(saliency, full), ptr(eig, full), ptr(neighbours, full)))
    return out_xyz, out_index, kept.value, flag, saliency, eig, neighbours


def cluster(min_points):
    def call(capi, ctx, n, full):
        return ctx.cluster_dbscan(cloud(n, 5), capi.cluster_params(radius=RADIUS, min_points=min_points), want_sizes=full, want_core=full, want_grouped=full)
    return call


def fpfh(capi, ctx, n, full):
    return as_tuple(ctx.fpfh_features(cloud(n, 6), unit(n, 7), K, want_counts=full, want_count=full))


def plane_system(capi, ctx, n, full):
    return ctx.plane_system(cloud(n, 2), cloud(n, 1), unit(n, 7), want_idx=full)


def gicp_system(capi, ctx, n, full):
    return ctx.gicp_system(cloud(n, 2), cov6(n, 8), cloud(n, 1), cov6(n, 9), want_idx=full)


def ndt_voxels(capi, ctx, n, full):
    xyz = cloud(n, 10)
    coord, mean, icov, rows = np.zeros((n, 3), np.int32), np.zeros((n, 3), np.float32), np.zeros((n, 6), np.float32), C.c_int(-1)
    count, cov, origin = np.zeros(n, np.int32), np.zeros((n, 6), np.float32), np.zeros(3, np.float32)
    capi._check(capi.ndt_voxels_raw(ctx._h, xyz.ctypes.data, n, NDT_VOXEL, None, NDT_MIN_POINTS, 0.01, coord.ctypes.data, mean.ctypes.data, icov.ctypes.data,
                                    C.addressof(rows), ptr(count, full), ptr(cov, full), ptr(origin, full)))
    return coord, mean, icov, rows.value, count, cov, origin


def ndt_system(capi, ctx, n, full):
    before, m = cloud(n, 2), ndt_map()
    coord, mean, icov = (np.ascontiguousarray(m[k]) for k in ("coord", "mean", "icov"))
    origin = np.ascontiguousarray(m["origin"], np.float32)
    sums, centre, idx, terms = np.zeros(32, np.float64), np.zeros(3, np.float32), np.zeros(n, np.int32), np.zeros(n, np.uint8)
    capi._check(capi.ndt_system_raw(ctx._h, before.ctypes.data, n, coord.ctypes.data, mean.ctypes.data, icov.ctypes.data, len(coord), m["voxel"],
                                    origin.ctypes.data, None, 7, 0.55, sums.ctypes.data, ptr(centre, full), ptr(idx, full), ptr(terms, full)))
    return sums, centre, idx, terms


def calls(capi):
    """name -> (the call, which new context serves as its reference)"""
    return {
        "knn_search-self": (knn_self, 0), "knn_search-queries": (knn_queries, 1), "estimate_normals": (normals, 0), "estimate_covariances": (covariances, 0),
        "remove_outliers-statistical": (outliers(capi.OUTLIER_STATISTICAL), 0), "remove_outliers-radius": (outliers(capi.OUTLIER_RADIUS), 1),
        "iss_keypoints": (iss, 0), "cluster_dbscan-min_points1": (cluster(1), 0), "cluster_dbscan-min_points3": (cluster(3), 1),
        "fpfh_features": (fpfh, 0), "plane_system": (plane_system, 0), "gicp_system": (gicp_system, 0), "ndt_voxels": (ndt_voxels, 0), "ndt_system": (ndt_system, 0),
    }


NAMES = ("knn_search-self", "knn_search-queries", "estimate_normals", "estimate_covariances", "remove_outliers-statistical", "remove_outliers-radius",
         "iss_keypoints", "cluster_dbscan-min_points1", "cluster_dbscan-min_points3", "fpfh_features", "plane_system", "gicp_system", "ndt_voxels", "ndt_system")


@functools.lru_cache(maxsize=None)
def fresh(group, n, full):
    """every call of `group` at (n, full), each on buffers no call has touched: one new context"""
    capi = load_package().capi
    with capi.Context(0) as new:
        return {name: call(capi, new, n, full) for name, (call, g) in calls(capi).items() if g == group}


@pytest.fixture(scope="module")
def used(capi):
    """the one context whose buffers grow, shrink and are skipped"""
    with capi.Context(0) as c:
        yield c


def same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        if isinstance(w, np.ndarray):
            if g.dtype != w.dtype or g.shape != w.shape or g.tobytes() != w.tobytes():
                return False
        elif g != w:
            return False
    return True


def test_ndt_voxels_case_has_a_distribution_at_its_smallest_size():
    """(CPU) at the smallest n of the sequence the cloud still has a voxel of NDT_MIN_POINTS points with a distribution, by the numpy restatement"""
    v = NR.voxels(cloud(min(SIZES), 10), NDT_VOXEL, min_points=NDT_MIN_POINTS)
    assert v["has"].any() and (v["count"][v["has"]] >= NDT_MIN_POINTS).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_used_context_answers_as_a_new_one(capi, used, name):
    assert set(NAMES) == set(calls(capi))
    call, group = calls(capi)[name]
    for full, sizes in ((True, SIZES), (False, SIZES), (True, (1000,))):
        for n in sizes:
            got = call(capi, used, n, full)
            assert same(got, fresh(group, n, full)[name]), "%s at n = %d, %s optional outputs: differs from a new context's answer" % (name, n, "all" if full else "no")
