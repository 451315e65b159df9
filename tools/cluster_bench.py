#!/usr/bin/env python3
"""mi_cluster_dbscan on a voxel-filtered surface (tools/iss_bench.py's: z = 0.6 sin(1.3 x) cos(1.1 y) + 0.01 noise over a square, seed 666,
through mi_voxel_downsample at voxel 0.2), host buffer in, labels, sizes and the grouping out.  Default: about 1e5 and 1e6 points.  The
radii are two and four times the cloud's resolution (mi_remove_outliers, statistical, k = 1: stats.mean), min_points 1 and 8.  Per size,
radius and min_points:
  the whole call (host clock, profiling off, median) and its stages with the stream drained after each (mi_cluster_dbscan_times,
  profiling on, median); the link kernel, K34, is the launch's own HIP-event time, the resolve kernel, K35, its stage's host time;
  the clusters, the largest one's share, the core and the noise points;
  beside it mi_remove_outliers in radius mode with its neighbours output (the FULL count) at the same radius on the same cloud: the same
  walk with a counter and nothing else, so K34 and K35 over that count kernel are the price of the union-find and of the border rule.
Per size once more: the link kernel on ONE component of the same size -- the same surface at four resolutions and min_points 1, asserted
to be a single cluster: every hook ends in one set, the worst case for contention.
One JSON line, in the field conventions of tests/golden/voxel_measured.json.
    python tools/cluster_bench.py [points ...]"""
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
from iss_bench import surface  # noqa: E402
from normals_bench import measure  # noqa: E402
from outlier_bench import OUTLIER_STAGES, outlier_run  # noqa: E402

CLUSTER_STAGES = ("workspace", "upload", "grid", "count", "link", "resolve", "finish", "total")


def one(capi, ctx, cloud, resolution, in_resolutions, min_points, count_kernel_ms):
    n = len(cloud)
    params = capi.cluster_params(radius=in_resolutions * resolution, min_points=min_points)
    labels, sizes, core, grouped = np.empty(n, np.int32), np.empty(n, np.int32), np.empty(n, np.uint8), np.empty(n, np.int32)
    n_clusters, n_grouped = C.c_int(0), C.c_int(0)
    full = measure(capi, ctx, lambda: capi.cluster_dbscan_raw(ctx._h, cloud.ctypes.data, n, C.addressof(params), labels.ctypes.data, C.addressof(n_clusters),
                                                             sizes.ctypes.data, n, None, grouped.ctypes.data, C.addressof(n_grouped)),
                   ctx.cluster_dbscan_times, CLUSTER_STAGES, n)
    rc = capi.cluster_dbscan_raw(ctx._h, cloud.ctypes.data, n, C.addressof(params), labels.ctypes.data, C.addressof(n_clusters), sizes.ctypes.data, n,
                                 core.ctypes.data, None, None)
    assert rc == capi.MI_OK and n_grouped.value == int((labels >= 0).sum()) == int(sizes[:n_clusters.value].sum())
    staged = full[2]
    return {"n": n, "radius_in_resolutions": in_resolutions, "radius": round(params.radius, 6), "min_points": min_points,
            "clusters": n_clusters.value, "largest_share": round(float(sizes[:n_clusters.value].max(initial=0)) / n, 4),
            "core_share": round(float(core.mean()), 4), "noise_share": round(float((labels < 0).mean()), 4),
            "call_ms": full[0], "call_ms_min": full[1], "staged_ms": staged,
            "link_ms": staged["link"], "link_ns_per_point": round(staged["link"] * 1e6 / n, 3),
            "resolve_ms": staged["resolve"], "resolve_ns_per_point": round(staged["resolve"] * 1e6 / n, 3),
            "radius_count_ms": count_kernel_ms, "link_over_radius_count": round(staged["link"] / count_kernel_ms, 3),
            "resolve_over_radius_count": round(staged["resolve"] / count_kernel_ms, 3)}


def size(capi, ctx, target):
    cloud = surface(ctx, target)
    n = len(cloud)
    _, _, stats = ctx.remove_outliers(cloud, capi.outlier_params(k=1), want_stats=True)
    resolution = float(stats.mean)
    rows = []
    for in_resolutions in (2, 4):
        rparams = capi.outlier_params(method=capi.OUTLIER_RADIUS, radius=in_resolutions * resolution, min_neighbours=1)
        run, _ = outlier_run(capi, ctx, cloud, rparams, True)
        rad = measure(capi, ctx, run, ctx.remove_outliers_times, OUTLIER_STAGES, n)
        for min_points in (1, 8):
            row = one(capi, ctx, cloud, resolution, in_resolutions, min_points, rad[2]["kernel"])
            row.update(resolution=round(resolution, 6), radius_count_call_ms=rad[0], call_over_radius_call=round(row["call_ms"] / rad[0], 3))
            rows.append(row)
    single = rows[2]                                                   # four resolutions, min_points 1
    assert single["clusters"] == 1 and single["largest_share"] == 1.0, "the surface at four resolutions is one component"
    return rows, {"n": n, "single_component_link_ms": single["link_ms"], "single_component_link_ns_per_point": single["link_ns_per_point"],
                  "single_component_link_over_radius_count": single["link_over_radius_count"]}


def main():
    capi = load_package().capi
    sizes = [int(float(a)) for a in sys.argv[1:]] or [10 ** 5, 10 ** 6]
    rows, singles = [], []
    with capi.Context(0) as ctx:
        ctx.preload()
        for target in sizes:
            r, s = size(capi, ctx, target)
            rows += r
            singles.append(s)
    print(json.dumps({"tool": "cluster_bench", "cloud": "voxel-filtered sine surface, seed 666, voxel 0.2; radii 2 and 4 resolutions; min_points 1 and 8; labels + sizes + grouping out",
                      "calls": "median of 7 whole calls after 2 warm-up calls and of 5 staged calls", "rows": rows, "single_component": singles}), flush=True)


if __name__ == "__main__":
    main()
