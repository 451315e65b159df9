#!/usr/bin/env python3
"""mi_remove_outliers on the synthetic uniform cloud (bench.synth_cloud: [-5, 5]^3, seed 666), host buffer in, kept points and indices
out.  Default: 1e5, 1e6 and 1e7 points.
  statistical  k = 8, 16, 32, beside mi_knn_search in self mode at the same k on the same cloud in the same process (idx only).  Per
               row, for either call: the whole call (host clock, profiling off, median) and its stages with the stream drained after each
               (mi_remove_outliers_times / mi_knn_search_times, profiling on, median; the kernel stage is the launch's own HIP-event
               time); then the score kernel over the search kernel and the whole call over the whole call.
  radius       a radius whose ball holds about 8 and about 32 points of the cloud (min_neighbours = half of that), with and without
               the neighbours output -- without it the count kernel leaves a point at min_neighbours.
One JSON line, in the field conventions of tests/golden/voxel_measured.json.
    python tools/outlier_bench.py [points ...]"""
import ctypes as C
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
for _v in ("OPENBLAS_NUM_THREADS", "OMP_NUM_THREADS", "MKL_NUM_THREADS"):   # see bench.quiet_host_pools: BLAS pools vs the CPU quota
    os.environ.setdefault(_v, "1")
import numpy as np  # noqa: E402
from __graft_entry__ import load_package  # noqa: E402
from bench import synth_cloud  # noqa: E402
from normals_bench import KNN_STAGES, measure  # noqa: E402

OUTLIER_STAGES = ("workspace", "upload", "check", "grid", "order", "kernel", "finish", "total")


def outlier_run(capi, ctx, cloud, params, want_neighbours):
    """(one whole call as a function returning the error code, the kept count it leaves)"""
    n = len(cloud)
    out_xyz, out_index, out_n = np.empty((n, 3), np.float32), np.empty(n, np.int32), C.c_int(0)
    neighbours = np.empty(n, np.int32) if want_neighbours else None
    run = lambda: capi.remove_outliers_raw(ctx._h, cloud.ctypes.data, n, C.addressof(params), out_xyz.ctypes.data, out_index.ctypes.data,
                                           C.addressof(out_n), None, None, None if neighbours is None else neighbours.ctypes.data, None)
    return run, out_n


def statistical(capi, ctx, cloud, k):
    n = len(cloud)
    idx = np.empty((n, k), np.int32)
    knn = measure(capi, ctx, lambda: capi.knn_search_raw(ctx._h, None, n, cloud.ctypes.data, n, k, capi.DIST_CPU_ROUNDING, float("inf"), idx.ctypes.data, None, None),
                  ctx.knn_search_times, KNN_STAGES, n)
    del idx
    run, out_n = outlier_run(capi, ctx, cloud, capi.outlier_params(k=k), False)
    out = measure(capi, ctx, run, ctx.remove_outliers_times, OUTLIER_STAGES, n)
    assert 0.9 * n <= out_n.value < n
    return {"method": "statistical", "n": n, "k": k, "kept": out_n.value, "call_ms": out[0], "call_ms_min": out[1], "staged_ms": out[2],
            "score_ns_per_point": round(out[2]["kernel"] * 1e6 / n, 3),
            "knn_call_ms": knn[0], "knn_call_ms_min": knn[1], "knn_staged_ms": knn[2], "knn_search_ns_per_point": round(knn[2]["search"] * 1e6 / n, 3),
            "score_over_knn_search": round(out[2]["kernel"] / knn[2]["search"], 3), "call_over_knn_call": round(out[0] / knn[0], 3)}


def radius(capi, ctx, cloud, inside, want_neighbours):
    n = len(cloud)
    r = (inside * 1000.0 / n * 3 / (4 * math.pi)) ** (1.0 / 3)              # the ball that holds `inside` of n points in [-5, 5]^3
    params = capi.outlier_params(method=capi.OUTLIER_RADIUS, radius=r, min_neighbours=inside // 2)
    run, out_n = outlier_run(capi, ctx, cloud, params, want_neighbours)
    out = measure(capi, ctx, run, ctx.remove_outliers_times, OUTLIER_STAGES, n)
    return {"method": "radius", "n": n, "points_in_ball": inside, "radius": round(r, 6), "min_neighbours": inside // 2, "neighbours_out": want_neighbours,
            "kept": out_n.value, "call_ms": out[0], "call_ms_min": out[1], "staged_ms": out[2], "count_ns_per_point": round(out[2]["kernel"] * 1e6 / n, 3)}


def main():
    capi = load_package().capi
    sizes = [int(float(a)) for a in sys.argv[1:]] or [10 ** 5, 10 ** 6, 10 ** 7]
    rows = []
    with capi.Context(0) as ctx:
        ctx.preload()
        for n in sizes:
            cloud = np.ascontiguousarray(synth_cloud(np, n)[0])
            for k in (8, 16, 32):
                rows.append(statistical(capi, ctx, cloud, k))
            for inside in (8, 32):
                for want_neighbours in (True, False):
                    rows.append(radius(capi, ctx, cloud, inside, want_neighbours))
    print(json.dumps({"tool": "outlier_bench", "cloud": "uniform [-5,5]^3, seed 666; kept points + indices out, idx out for the k-NN call",
                      "calls": "median of 7 whole calls after 2 warm-up calls and of 5 staged calls (1e7 points: 5 after 1, and 5)", "rows": rows}), flush=True)


if __name__ == "__main__":
    main()
