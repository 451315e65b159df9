#!/usr/bin/env python3
"""mi_icp_gicp_register beside mi_icp_plane_register on the scan-like pair of tools/plane_icp_bench.py: both clouds drawn from the surface
z = 0.3 sin(1.5 x) cos(1.2 y) (plus 2 mm of noise) and passed through mi_voxel_downsample at a 0.02 voxel, the moving cloud 2 degrees and
0.02 off; covariances of both clouds from mi_estimate_covariances (MI_COV_PLANE, epsilon 1e-3, k = 16), the fixed cloud's normals from
mi_estimate_normals at the same k.  Default: about 1e5 and 1e6 points per cloud.  Per size, one JSON row with, for both methods:
  the whole call (host clock, profiling off, median) and its stages with the stream drained after each (profiling on);
  ms per iteration of the step kernel and of the reduce-and-solve launches (profiling on, sync_every = 1 so that no launch is an empty one
  behind the stop; mi_profile_get books them under "nn" and "solve");
  the iteration count, the stop reason and the distance from the ground truth;
and mi_estimate_covariances beside mi_estimate_normals (whole call and the fused kernel).
    python tools/gicp_bench.py [--out FILE] [points ...]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
for _v in ("OPENBLAS_NUM_THREADS", "OMP_NUM_THREADS", "MKL_NUM_THREADS"):   # see bench.quiet_host_pools: BLAS pools vs the CPU quota
    os.environ.setdefault(_v, "1")
import numpy as np  # noqa: E402
from __graft_entry__ import load_package  # noqa: E402
from plane_icp_bench import STAGES, VOXEL, median, pair  # noqa: E402

K_NEIGHBOURS, EPSILON = 16, 1e-3


def timed(call, repeat=7, warm=2):
    out, ms = None, []
    for i in range(warm + repeat):
        t0 = time.perf_counter()
        out = call()
        if i >= warm:
            ms.append((time.perf_counter() - t0) * 1e3)
    return out, ms


def registration(capi, ctx, G, limit, register, times):
    """register(params) -> (R, t, iterations, error, stop): one method's figures"""
    (R, t, it, err, why), call = timed(lambda: register(capi.plane_params(max_distance_squared=limit)))
    ctx.profile_enable(True)
    ctx.profile_reset()
    staged = {s: [] for s in STAGES}
    for _ in range(5):
        register(capi.plane_params(max_distance_squared=limit, sync_every=1))
        now = times()
        for s in STAGES:
            staged[s].append(now[s])
    step_ms, step_n = ctx.profile_get(capi.KERNEL_NN)
    solve_ms, solve_n = ctx.profile_get(capi.KERNEL_SOLVE)
    ctx.profile_enable(False)
    ctx.profile_reset()
    return {"call_ms": round(median(call), 4), "call_ms_min": round(min(call), 4), "staged_ms": {s: round(median(v), 4) for s, v in staged.items()},
            "step_kernel_ms_per_iteration": round(step_ms / step_n, 5), "reduce_solve_ms_per_iteration": round(solve_ms / solve_n, 5),
            "launches_timed": [int(step_n), int(solve_n)], "iterations": it, "stop_reason": why, "error": float(err),
            "off_truth_dR_dt": [float(np.abs(R - G[:3, :3]).max()), float(np.abs(t - G[:3, 3]).max())]}


def one(capi, ctx, target):
    moving, fixed, normals, G = pair(ctx, target)
    limit = (5 * VOXEL) ** 2
    cov_a, cov_ms = timed(lambda: ctx.estimate_covariances(fixed, K_NEIGHBOURS, capi.COV_PLANE, EPSILON), repeat=5, warm=1)
    _, normals_ms = timed(lambda: ctx.estimate_normals(fixed, K_NEIGHBOURS), repeat=5, warm=1)
    cov_b = ctx.estimate_covariances(moving, K_NEIGHBOURS, capi.COV_PLANE, EPSILON)
    ctx.profile_enable(True)
    ctx.estimate_normals(fixed, K_NEIGHBOURS)
    normals_kernel = ctx.estimate_normals_times()["fused"]
    ctx.profile_enable(False)
    gicp = registration(capi, ctx, G, limit, lambda p: ctx.icp_gicp_register(moving, cov_b, fixed, cov_a, p), ctx.icp_gicp_times)
    plane = registration(capi, ctx, G, limit, lambda p: ctx.icp_plane_register(moving, fixed, normals, p), ctx.icp_plane_times)
    return {"target": target, "n_moving": len(moving), "m_fixed": len(fixed), "gicp": gicp, "plane": plane,
            "step_kernel_gicp_over_plane": round(gicp["step_kernel_ms_per_iteration"] / plane["step_kernel_ms_per_iteration"], 3),
            "estimate_covariances_call_ms": round(median(cov_ms), 4), "estimate_normals_call_ms": round(median(normals_ms), 4),
            "estimate_normals_kernel_ms": round(normals_kernel, 5)}


def main():
    args = sys.argv[1:]
    out = None
    if "--out" in args:
        out = args[args.index("--out") + 1]
        del args[args.index("--out"):args.index("--out") + 2]
    capi = load_package().capi
    sizes = [int(float(a)) for a in args] or [10 ** 5, 10 ** 6]
    rows = []
    with capi.Context(0) as ctx:
        ctx.preload()
        for target in sizes:
            rows.append(one(capi, ctx, target))
    doc = {"tool": "gicp_bench", "pair": "z = 0.3 sin(1.5 x) cos(1.2 y) + 2 mm noise, voxel 0.02; covariances MI_COV_PLANE epsilon 1e-3 k = 16, normals k = 16; "
                                         "start 2 degrees and 0.02 off; limit (5 voxels)^2",
           "calls": "median of 7 whole calls after 2 warm-up calls; 5 staged and profiled calls per method", "rows": rows}
    print(json.dumps(doc), flush=True)
    if out:
        with open(out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
