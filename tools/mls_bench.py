#!/usr/bin/env python3
"""mi_mls_smooth on a voxel-filtered noisy surface (tools/iss_bench.py's: z = 0.6 sin(1.3 x) cos(1.1 y) + 0.01 noise over a square, seed
666, through mi_voxel_downsample at voxel 0.2), self mode, host buffer in, smoothed points and normals out.  Default: about 1e5 and 1e6
points.  The radii are four and six times the cloud's resolution (mi_remove_outliers, statistical, k = 1: stats.mean).  Per size, radius
and order (1 and 2):
  the whole call (host clock, profiling off, median) and its stages with the stream drained after each (mi_mls_smooth_times, profiling on,
  median; the fit stage, K50, is the launch's own HIP-event time: the kernel alone);
  the mean size of the ball, the share of the points each status took, and the RMS distance to the noise-free surface before and after;
  beside it mi_iss_keypoints with that radius as its salient radius on the same cloud: its saliency kernel K32 does ONE walk with a
  scatter, so K50 over K32 is the price of the second walk and the solve (order 2) or of the plane and the frame alone (order 1);
and per size mi_estimate_normals at k = 16 on the same cloud, whole call and fused kernel.
One JSON line, in the field conventions of tests/golden/voxel_measured.json.
    python tools/mls_bench.py [points ...]"""
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
from iss_bench import ISS_STAGES, surface  # noqa: E402
from normals_bench import NORMALS_STAGES, measure  # noqa: E402

MLS_STAGES = ("workspace", "upload", "check", "grid", "order", "fit", "download", "total")


def surface_rms(p):
    """RMS distance of points to the noise-free surface, to first order: the height's residual over the gradient's length"""
    p = np.asarray(p, np.float64)
    x, y = p[:, 0], p[:, 1]
    f = 0.6 * np.sin(1.3 * x) * np.cos(1.1 * y)
    fx, fy = 0.78 * np.cos(1.3 * x) * np.cos(1.1 * y), -0.66 * np.sin(1.3 * x) * np.sin(1.1 * y)
    return float(np.sqrt((((p[:, 2] - f) ** 2) / (1 + fx * fx + fy * fy)).mean()))


def one(capi, ctx, cloud, resolution, factor, order, iss):
    n = len(cloud)
    params = capi.mls_params(radius=factor * resolution, order=order)
    xyz, normals = np.empty((n, 3), np.float32), np.empty((n, 3), np.float32)
    full = measure(capi, ctx, lambda: capi.mls_smooth_raw(ctx._h, cloud.ctypes.data, n, None, n, C.addressof(params), xyz.ctypes.data, normals.ctypes.data,
                                                          None, None, None),
                   ctx.mls_smooth_times, MLS_STAGES, n)
    out, neighbours, status = ctx.mls_smooth(cloud, params, want_neighbours=True, want_status=True)
    assert np.array_equal(out.view(np.uint32), xyz.view(np.uint32))
    share = np.bincount(status, minlength=3) / n
    return {"n": n, "radius_in_resolutions": factor, "radius": round(params.radius, 6), "order": order, "mean_ball": round(float(neighbours.mean()), 2),
            "quadratic_share": round(float(share[0]), 4), "plane_share": round(float(share[1]), 4), "untouched_share": round(float(share[2]), 4),
            "rms_before": round(surface_rms(cloud), 6), "rms_after": round(surface_rms(out), 6),
            "call_ms": full[0], "call_ms_min": full[1], "staged_ms": full[2], "k50_ms": full[2]["fit"], "k50_ns_per_point": round(full[2]["fit"] * 1e6 / n, 3),
            "k32_ms": iss[2]["saliency"], "k50_over_k32": round(full[2]["fit"] / iss[2]["saliency"], 3), "iss_call_ms": iss[0]}


def main():
    capi = load_package().capi
    sizes = [int(float(a)) for a in sys.argv[1:]] or [10 ** 5, 10 ** 6]
    rows, normals_rows = [], []
    with capi.Context(0) as ctx:
        ctx.preload()
        for target in sizes:
            cloud = surface(ctx, target)
            n = len(cloud)
            _, _, stats = ctx.remove_outliers(cloud, capi.outlier_params(k=1), want_stats=True)
            resolution = float(stats.mean)
            for factor in (4, 6):
                ip = capi.iss_params(salient_radius=factor * resolution, non_max_radius=factor * resolution)
                out_n = C.c_int(0)
                iss = measure(capi, ctx, lambda: capi.iss_keypoints_raw(ctx._h, cloud.ctypes.data, n, C.addressof(ip), None, None, C.addressof(out_n), None, None, None, None),
                              ctx.iss_keypoints_times, ISS_STAGES, n)
                for order in (1, 2):
                    rows.append(dict(one(capi, ctx, cloud, resolution, factor, order, iss), resolution=round(resolution, 6)))
            nrm, curv = np.empty((n, 3), np.float32), np.empty(n, np.float32)
            est = measure(capi, ctx, lambda: capi.estimate_normals_raw(ctx._h, cloud.ctypes.data, n, 16, capi.DIST_CPU_ROUNDING, float("inf"), None, nrm.ctypes.data,
                                                                      curv.ctypes.data, None),
                          ctx.estimate_normals_times, NORMALS_STAGES, n)
            normals_rows.append({"n": n, "k": 16, "call_ms": est[0], "call_ms_min": est[1], "fused_ms": est[2]["fused"]})
    print(json.dumps({"tool": "mls_bench", "cloud": "voxel-filtered sine surface, seed 666, voxel 0.2; self mode; radii 4 and 6 resolutions; points + normals out",
                      "calls": "median of 7 whole calls after 2 warm-up calls and of 5 staged calls", "rows": rows, "estimate_normals": normals_rows}), flush=True)


if __name__ == "__main__":
    main()
