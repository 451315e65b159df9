#!/usr/bin/env python3
"""mi_icp_plane_register on a scan-like pair: both clouds drawn from the surface z = 0.3 sin(1.5 x) cos(1.2 y) (plus 2 mm of noise) and
passed through mi_voxel_downsample at a 0.02 voxel, the fixed cloud's normals from mi_estimate_normals (k = 16, turned upwards), the moving
cloud 2 degrees and 0.02 off.  Default: about 1e5 and 1e6 points per cloud.  Per size, one JSON row:
  the whole call (host clock, profiling off, median) and its stages with the stream drained after each (mi_icp_plane_times, profiling on);
  ms per iteration of the step kernel and of the reduce-and-solve launches (profiling on, sync_every = 1 so that no launch is an empty one
  behind the stop; mi_profile_get books them under "nn" and "solve"), beside the search stage of mi_knn_search with k = 1 and the moving
  cloud as separate queries on the same clouds and grid -- the search the step kernel contains, so the difference is the price of the sums;
  the iteration count and the distance from the ground truth, beside mi_icp_register (point-to-point) on the same pair.
    python tools/plane_icp_bench.py [points ...]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
for _v in ("OPENBLAS_NUM_THREADS", "OMP_NUM_THREADS", "MKL_NUM_THREADS"):   # see bench.quiet_host_pools: BLAS pools vs the CPU quota
    os.environ.setdefault(_v, "1")
import numpy as np  # noqa: E402
from __graft_entry__ import load_package  # noqa: E402

VOXEL = 0.02
STAGES = ("workspace", "upload", "check", "grid", "order", "iterations", "download", "total")


def median(v):
    return float(np.median(np.asarray(v, np.float64)))


def rodrigues(w):
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    return np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * (K @ K)


def draw(rng, side, count):
    xy = rng.uniform(-side / 2, side / 2, (count, 2))
    z = 0.3 * np.sin(1.5 * xy[:, 0]) * np.cos(1.2 * xy[:, 1]) + rng.normal(0, 0.002, count)
    return np.concatenate([xy, z[:, None]], axis=1)


def pair(ctx, target):
    """(moving, fixed, normals, ground truth [4, 4]): about `target` points each after the voxel filter"""
    rng = np.random.default_rng(666)
    side = float(np.sqrt(target) * VOXEL)
    Rg = rodrigues(np.deg2rad(2.0) * np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0))
    tg = 0.02 * np.array([0.6, -0.48, 0.64])
    fixed = ctx.voxel_downsample(draw(rng, side, 3 * target).astype(np.float32), VOXEL)
    raw = draw(rng, side, 3 * target)
    moving = ctx.voxel_downsample(((raw - tg) @ Rg).astype(np.float32), VOXEL)            # G^-1 of a second draw of the same surface
    normals = ctx.estimate_normals(fixed, 16, viewpoint=np.array([0, 0, 1e4], np.float32))
    G = np.eye(4)
    G[:3, :3], G[:3, 3] = Rg, tg
    return np.ascontiguousarray(moving), np.ascontiguousarray(fixed), normals, G


def one(capi, ctx, target):
    moving, fixed, normals, G = pair(ctx, target)
    limit = (5 * VOXEL) ** 2
    p = capi.plane_params(max_distance_squared=limit)
    call = []
    for i in range(2 + 7):
        t0 = time.perf_counter()
        R, t, it, err, why = ctx.icp_plane_register(moving, fixed, normals, p)
        if i >= 2:
            call.append((time.perf_counter() - t0) * 1e3)
    ctx.profile_enable(True)
    staged = {s: [] for s in STAGES}
    p1 = capi.plane_params(max_distance_squared=limit, sync_every=1)
    ctx.profile_reset()
    for _ in range(5):
        ctx.icp_plane_register(moving, fixed, normals, p1)
        times = ctx.icp_plane_times()
        for s in STAGES:
            staged[s].append(times[s])
    step_ms, step_n = ctx.profile_get(capi.KERNEL_NN)
    solve_ms, solve_n = ctx.profile_get(capi.KERNEL_SOLVE)
    search = []
    for _ in range(5):
        ctx.knn_search(moving, fixed, 1, max_d2=limit, want_d2=False)
        search.append(ctx.knn_search_times()["search"])
    ctx.profile_enable(False)
    ctx.profile_reset()
    Rp, tp, itp, errp = ctx.icp_register(moving, fixed, capi.icp_params(eps=1e-9, max_iterations=50, max_distance_squared=limit))

    def off(R_, t_):
        return [float(np.abs(R_ - G[:3, :3]).max()), float(np.abs(t_ - G[:3, 3]).max())]

    return {"target": target, "n_moving": len(moving), "m_fixed": len(fixed), "call_ms": round(median(call), 4), "call_ms_min": round(min(call), 4),
            "staged_ms": {s: round(median(v), 4) for s, v in staged.items()},
            "step_kernel_ms_per_iteration": round(step_ms / step_n, 5), "reduce_solve_ms_per_iteration": round(solve_ms / solve_n, 5),
            "launches_timed": [int(step_n), int(solve_n)], "knn_k1_search_ms": round(median(search), 5),
            "step_over_knn_search": round(step_ms / step_n / median(search), 3),
            "iterations": it, "stop_reason": why, "error": float(err), "off_truth_dR_dt": off(R, t),
            "point_to_point": {"iterations": itp, "error": float(errp), "off_truth_dR_dt": off(Rp, tp)}}


def main():
    capi = load_package().capi
    sizes = [int(float(a)) for a in sys.argv[1:]] or [10 ** 5, 10 ** 6]
    rows = []
    with capi.Context(0) as ctx:
        ctx.preload()
        for target in sizes:
            rows.append(one(capi, ctx, target))
    print(json.dumps({"tool": "plane_icp_bench", "pair": "z = 0.3 sin(1.5 x) cos(1.2 y) + 2 mm noise, voxel 0.02, normals k = 16; start 2 degrees and 0.02 off; limit (5 voxels)^2",
                      "calls": "median of 7 whole calls after 2 warm-up calls; 5 staged and profiled calls", "rows": rows}), flush=True)


if __name__ == "__main__":
    main()
