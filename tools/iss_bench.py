#!/usr/bin/env python3
"""mi_iss_keypoints on a voxel-filtered surface (z = 0.6 sin(1.3 x) cos(1.1 y) + 0.01 noise over a square, seed 666, through
mi_voxel_downsample at voxel 0.2), host buffer in, keypoints and indices out.  Default: about 1e5 and 1e6 points.  The radii are six and
four times the cloud's resolution (mi_remove_outliers, statistical, k = 1: stats.mean).  Per size:
  the whole call (host clock, profiling off, median) and its stages with the stream drained after each (mi_iss_keypoints_times,
  profiling on, median; the saliency stage, K32, is the launch's own HIP-event time);
  K33 on its own: the finish stage of a call that asks for no output but the count, i.e. K33, the two counting launches of the
  compaction and the read-back of one state block;
  the candidates' and the keypoints' share of the points, and the mean size of the salient ball;
  beside it mi_remove_outliers in radius mode with its neighbours output at the salient radius on the same cloud: the same walk with a
  counter where K32 has nine fp64 sums, so K32 over that count kernel is the price of the scatter matrix.
One JSON line, in the field conventions of tests/golden/voxel_measured.json.
    python tools/iss_bench.py [points ...]"""
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
from normals_bench import measure  # noqa: E402
from outlier_bench import OUTLIER_STAGES, outlier_run  # noqa: E402

ISS_STAGES = ("workspace", "upload", "check", "grid", "order", "saliency", "finish", "total")
VOXEL = 0.2


def surface(ctx, target):
    """about `target` points: three raw points per voxel of a square of target voxels, then the voxel filter"""
    rng = np.random.default_rng(666)
    half = 0.5 * VOXEL * math.sqrt(target)
    xy = rng.uniform(-half, half, (3 * target, 2))
    z = 0.6 * np.sin(1.3 * xy[:, 0]) * np.cos(1.1 * xy[:, 1]) + 0.01 * rng.normal(size=len(xy))
    raw = np.concatenate([xy, z[:, None]], axis=1).astype(np.float32)
    return np.ascontiguousarray(ctx.voxel_downsample(raw, VOXEL))


def one(capi, ctx, target):
    cloud = surface(ctx, target)
    n = len(cloud)
    _, _, stats = ctx.remove_outliers(cloud, capi.outlier_params(k=1), want_stats=True)
    resolution = float(stats.mean)
    params = capi.iss_params(salient_radius=6 * resolution, non_max_radius=4 * resolution)
    out_xyz, out_index, out_n = np.empty((n, 3), np.float32), np.empty(n, np.int32), C.c_int(0)
    full = measure(capi, ctx, lambda: capi.iss_keypoints_raw(ctx._h, cloud.ctypes.data, n, C.addressof(params), out_xyz.ctypes.data, out_index.ctypes.data,
                                                             C.addressof(out_n), None, None, None, None),
                   ctx.iss_keypoints_times, ISS_STAGES, n)
    keypoints = out_n.value
    bare = measure(capi, ctx, lambda: capi.iss_keypoints_raw(ctx._h, cloud.ctypes.data, n, C.addressof(params), None, None, C.addressof(out_n), None, None, None, None),
                   ctx.iss_keypoints_times, ISS_STAGES, n)
    assert out_n.value == keypoints
    _, _, saliency, neighbours = ctx.iss_keypoints(cloud, params, want_saliency=True, want_neighbours=True)
    rparams = capi.outlier_params(method=capi.OUTLIER_RADIUS, radius=params.salient_radius, min_neighbours=params.min_neighbours)
    run, _ = outlier_run(capi, ctx, cloud, rparams, True)
    rad = measure(capi, ctx, run, ctx.remove_outliers_times, OUTLIER_STAGES, n)
    return {"n": n, "resolution": round(resolution, 6), "salient_radius": round(params.salient_radius, 6), "non_max_radius": round(params.non_max_radius, 6),
            "mean_salient_ball": round(float(neighbours.mean()), 2), "candidates": int((saliency > 0).sum()), "keypoints": keypoints,
            "candidate_share": round(float((saliency > 0).mean()), 4), "keypoint_share": round(keypoints / n, 5),
            "call_ms": full[0], "call_ms_min": full[1], "staged_ms": full[2],
            "k32_ms": full[2]["saliency"], "k32_ns_per_point": round(full[2]["saliency"] * 1e6 / n, 3),
            "k33_ms": bare[2]["finish"], "k33_ns_per_point": round(bare[2]["finish"] * 1e6 / n, 3),
            "radius_count_call_ms": rad[0], "radius_count_staged_ms": rad[2], "radius_count_ns_per_point": round(rad[2]["kernel"] * 1e6 / n, 3),
            "k32_over_radius_count": round(full[2]["saliency"] / rad[2]["kernel"], 3), "call_over_radius_call": round(full[0] / rad[0], 3)}


def main():
    capi = load_package().capi
    sizes = [int(float(a)) for a in sys.argv[1:]] or [10 ** 5, 10 ** 6]
    rows = []
    with capi.Context(0) as ctx:
        ctx.preload()
        for target in sizes:
            rows.append(one(capi, ctx, target))
    print(json.dumps({"tool": "iss_bench", "cloud": "voxel-filtered sine surface, seed 666, voxel 0.2; radii 6 and 4 resolutions; keypoints + indices out",
                      "calls": "median of 7 whole calls after 2 warm-up calls and of 5 staged calls", "rows": rows}), flush=True)


if __name__ == "__main__":
    main()
