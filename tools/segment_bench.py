#!/usr/bin/env python3
"""mi_segment_plane on a synthetic room: a floor (50 % of the points), two walls (15 % each) and uniform clutter (20 %) in a box of
10 x 10 x 4, Gaussian noise of 0.01 on the planes, seed 666, host buffer in, planes, counts and labels out.  Default: about 1e5 and 1e6
points; 1 000 and 10 000 hypotheses per plane; one plane and four planes (distance_threshold 0.04, 2 refinement steps, min_inliers 1 % of
the cloud).  Per size, H and planes:
  the whole call (host clock, profiling off, median) and its stages with the stream drained after each, summed over the rounds
  (mi_segment_plane_times, profiling on, median); the planes found and their sizes; point tests per ns of the counting kernel, K40;
  beside the one-plane rows ransac_count, K24, at the same H x C as the yardstick: mi_ransac_register on the cloud paired with itself (every
  point a correspondence, no edge rule, so every hypothesis is valid and none is skipped), its `count` stage.
One JSON line, in the field conventions of tests/golden/voxel_measured.json.
    python tools/segment_bench.py [points ...]"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
for _v in ("OPENBLAS_NUM_THREADS", "OMP_NUM_THREADS", "MKL_NUM_THREADS"):   # see bench.quiet_host_pools: BLAS pools vs the CPU quota
    os.environ.setdefault(_v, "1")
import numpy as np  # noqa: E402
from __graft_entry__ import load_package  # noqa: E402
from normals_bench import measure  # noqa: E402

SEGMENT_STAGES = ("workspace", "upload", "check", "hypotheses", "count", "argmax", "refine", "total")
RANSAC_STAGES = ("workspace", "upload", "hypotheses", "count", "argmax", "refine", "unused6", "total")
THRESHOLD = 0.04


def room(n, seed=666):
    rng = np.random.default_rng(seed)
    nf, nw = n // 2, 3 * n // 20
    noise = lambda k: 0.01 * rng.normal(size=k)                                   # noqa: E731
    floor = np.stack([rng.uniform(0, 10, nf), rng.uniform(0, 10, nf), noise(nf)], axis=1)
    wall_x = np.stack([noise(nw), rng.uniform(0, 10, nw), rng.uniform(0, 4, nw)], axis=1)
    wall_y = np.stack([rng.uniform(0, 10, nw), noise(nw), rng.uniform(0, 4, nw)], axis=1)
    clutter = rng.uniform([0, 0, 0], [10, 10, 4], (n - nf - 2 * nw, 3))
    cloud = np.concatenate([floor, wall_x, wall_y, clutter]).astype(np.float32)
    return np.ascontiguousarray(cloud[rng.permutation(n)])


def one(capi, ctx, cloud, hyp, planes, yardstick_ms):
    n = len(cloud)
    out, inl, labels, found = np.empty((16, 4), np.float32), np.empty(16, np.int32), np.empty(n, np.int32), C.c_int(0)
    run = lambda: capi.segment_plane_raw(ctx._h, cloud.ctypes.data, n, THRESHOLD, hyp, 1, 2, planes, max(n // 100, 3), None, 0.0, out.ctypes.data,   # noqa: E731
                                         C.addressof(found), inl.ctypes.data, labels.ctypes.data, None, None)
    full = measure(capi, ctx, run, ctx.segment_plane_times, SEGMENT_STAGES, n)
    staged, k = full[2], found.value
    tests = float(hyp) * float(n if planes == 1 else n + sum(n - int(inl[:p + 1].sum()) for p in range(k - 1)))
    row = {"n": n, "hypotheses": hyp, "max_planes": planes, "planes": k, "plane_inliers": inl[:k].tolist(), "unlabelled_share": round(float((labels < 0).mean()), 4),
           "call_ms": full[0], "call_ms_min": full[1], "staged_ms": staged, "count_ms": staged["count"],
           "point_tests_per_ns": round(tests / (staged["count"] * 1e6), 1) if staged["count"] > 0 else None}
    if yardstick_ms is not None:
        row.update(ransac_count_ms=yardstick_ms, count_over_ransac_count=round(staged["count"] / yardstick_ms, 3) if yardstick_ms > 0 else None)
    return row


def ransac_count_ms(capi, ctx, cloud, hyp):
    """K24 at the same H x C: the cloud paired with itself"""
    n = len(cloud)
    idx = np.arange(n, dtype=np.int32)
    params = capi.ransac_params(THRESHOLD, hypotheses=hyp, seed=1, edge_similarity=0.0, refine_iterations=0)
    R9, t3 = np.empty(9, np.float32), np.empty(3, np.float32)
    inl, best, nvalid, rmse = C.c_int(0), C.c_int(0), C.c_int(0), C.c_float(0)
    run = lambda: capi.ransac_register_raw(ctx._h, cloud.ctypes.data, n, cloud.ctypes.data, n, idx.ctypes.data, C.addressof(params), R9.ctypes.data,   # noqa: E731
                                           t3.ctypes.data, C.addressof(inl), C.addressof(rmse), C.addressof(best), C.addressof(nvalid), None)
    return measure(capi, ctx, run, ctx.ransac_register_times, RANSAC_STAGES, n)[2]["count"]


def main(argv):
    sizes = [int(a) for a in argv] or [100_000, 1_000_000]
    capi = load_package().capi
    rows = []
    with capi.Context(0) as ctx:
        ctx.preload()
        for n in sizes:
            cloud = room(n)
            for hyp in (1000, 10000):
                yard = ransac_count_ms(capi, ctx, cloud, hyp)
                rows.append(one(capi, ctx, cloud, hyp, 1, yard))
                rows.append(one(capi, ctx, cloud, hyp, 4, None))
    print(json.dumps({"tool": "segment_bench", "distance_threshold": THRESHOLD, "rows": rows}))


if __name__ == "__main__":
    main(sys.argv[1:])
