#!/usr/bin/env python3
"""mi_radius_search on a voxel-filtered surface (tools/iss_bench.py's: z = 0.6 sin(1.3 x) cos(1.1 y) + 0.01 noise over a square, seed 666,
through mi_voxel_downsample at voxel 0.2), self mode, host buffer in, offsets, idx and d2 out at a capacity that fits.  Default: about 1e5
and 1e6 points.  The radii are those whose disc on the surface holds about 8 and about 32 points (pi r^2 = points x resolution^2 / the
cloud's points per resolution^2, solved from the cloud's own density).  Per size and radius:
  the whole call, sorted and unsorted and counts only (host clock, profiling off: median, minimum and maximum of the timed calls after the
  warm-up calls) and the sorted call's stages with the stream drained after each (mi_radius_search_times, profiling on, median): the count
  kernel, the fill kernel K52 and the sort kernel K53 are the launches' own HIP-event times, the other stages host time;
  the mean and the longest row;
  beside it mi_remove_outliers in radius mode with its neighbours output (the FULL count) at the same radius on the same cloud: the same
  walk with a counter and nothing else -- the price of one walk -- and mi_knn_search at k = 8 and k = 32 under the limit radius^2: what a
  caller had before.
One JSON line, in the field conventions of tests/golden/voxel_measured.json.
    python tools/radius_bench.py [points ...]"""
import ctypes as C
import json
import math
import os
import sys
import time
from statistics import median

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
for _v in ("OPENBLAS_NUM_THREADS", "OMP_NUM_THREADS", "MKL_NUM_THREADS"):   # see bench.quiet_host_pools: BLAS pools vs the CPU quota
    os.environ.setdefault(_v, "1")
import numpy as np  # noqa: E402
from __graft_entry__ import load_package  # noqa: E402
from iss_bench import surface  # noqa: E402
from normals_bench import KNN_STAGES, measure, repeats  # noqa: E402
from outlier_bench import OUTLIER_STAGES, outlier_run  # noqa: E402

RADIUS_STAGES = ("workspace", "front", "count", "scan", "fill", "sort", "download", "total")


def spread(capi, run, n):
    """run() is one whole call returning the error code: (median, minimum, maximum) of the timed calls, in ms"""
    warm, calls, _ = repeats(n)
    got = []
    for i in range(warm + calls):
        t0 = time.perf_counter()
        rc = run()
        if i >= warm:
            got.append((time.perf_counter() - t0) * 1e3)
        assert rc == capi.MI_OK, capi.lib().mi_last_error()
    return round(median(got), 4), round(min(got), 4), round(max(got), 4)


def one(capi, ctx, cloud, radius, inside):
    n = len(cloud)
    offsets, total = ctx.radius_count(cloud, radius)
    lengths = np.diff(offsets)
    idx, d2, got = np.empty(total, np.int32), np.empty(total, np.float32), C.c_longlong(0)

    def call(srt, lists=True):
        return lambda: capi.radius_search_raw(ctx._h, None, n, cloud.ctypes.data, n, radius, capi.DIST_CPU_ROUNDING, srt, offsets.ctypes.data,
                                              idx.ctypes.data if lists else None, d2.ctypes.data if lists else None, total if lists else 0, C.addressof(got))

    full = measure(capi, ctx, call(1), ctx.radius_search_times, RADIUS_STAGES, n)
    assert got.value == total
    staged = full[2]
    sorted_ms, unsorted_ms, counts_ms = spread(capi, call(1), n), spread(capi, call(0), n), spread(capi, call(1, False), n)
    params = capi.outlier_params(method=capi.OUTLIER_RADIUS, radius=radius, min_neighbours=1)
    run, _ = outlier_run(capi, ctx, cloud, params, True)
    rad = measure(capi, ctx, run, ctx.remove_outliers_times, OUTLIER_STAGES, n)
    row = {"n": n, "points_in_ball_aimed_at": inside, "radius": round(radius, 6), "total": total, "mean_row": round(float(lengths.mean()), 3),
           "longest_row": int(lengths.max()), "call_ms_sorted_median_min_max": sorted_ms, "call_ms_unsorted_median_min_max": unsorted_ms,
           "call_ms_counts_only_median_min_max": counts_ms, "staged_ms": staged,
           "count_ns_per_query": round(staged["count"] * 1e6 / n, 3), "fill_ns_per_entry": round(staged["fill"] * 1e6 / total, 4),
           "sort_ns_per_entry": round(staged["sort"] * 1e6 / total, 4),
           "fill_over_count": round(staged["fill"] / staged["count"], 3), "sort_over_count": round(staged["sort"] / staged["count"], 3),
           "dominant": "fill" if staged["fill"] >= staged["sort"] else "sort",
           "radius_count_kernel_ms": rad[2]["kernel"], "radius_count_call_ms": rad[0], "call_over_radius_count_call": round(sorted_ms[0] / rad[0], 3)}
    r2 = float(np.float32(radius) * np.float32(radius))
    for k in (8, 32):
        kidx = np.empty((n, k), np.int32)
        kd2 = np.empty((n, k), np.float32)
        knn = measure(capi, ctx, lambda: capi.knn_search_raw(ctx._h, None, n, cloud.ctypes.data, n, k, capi.DIST_CPU_ROUNDING, r2, kidx.ctypes.data, kd2.ctypes.data, None),
                      ctx.knn_search_times, KNN_STAGES, n)
        row["knn_k%d_call_ms" % k], row["knn_k%d_search_ms" % k] = knn[0], knn[2]["search"]
        row["rows_cut_short_by_k%d" % k] = round(float((lengths > k).mean()), 4)
    return row


def main():
    capi = load_package().capi
    sizes = [int(float(a)) for a in sys.argv[1:]] or [10 ** 5, 10 ** 6]
    rows = []
    with capi.Context(0) as ctx:
        ctx.preload()
        for target in sizes:
            cloud = surface(ctx, target)
            # the surface's density from a probe count: points per unit disc area at a radius of five voxels
            _, probe_total = ctx.radius_count(cloud, 1.0)
            per_area = probe_total / len(cloud) / math.pi
            for inside in (8, 32):
                rows.append(one(capi, ctx, cloud, math.sqrt(inside / (math.pi * per_area)), inside))
    print(json.dumps({"tool": "radius_bench", "cloud": "voxel-filtered sine surface, seed 666, voxel 0.2; self mode; offsets + idx + d2 out",
                      "calls": "median, minimum and maximum of 7 whole calls after 2 warm-up calls; stages: median of 5 staged calls", "rows": rows}), flush=True)


if __name__ == "__main__":
    main()
