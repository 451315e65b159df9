#!/usr/bin/env python3
"""mi_ndt_register beside mi_icp_gicp_register, and mi_ndt_voxels beside mi_voxel_downsample, on the scan-like pair of
tools/plane_icp_bench.py: both clouds drawn from the surface z = 0.3 sin(1.5 x) cos(1.2 y) (plus 2 mm of noise) and passed through
mi_voxel_downsample at a 0.02 voxel, the moving cloud 2 degrees and 0.02 off.  The NDT map is mi_ndt_voxels of the fixed cloud at a voxel
of 0.2 (ten point spacings; min_points 6, eig_ratio 0.01); generalized ICP runs with the covariances of tools/gicp_bench.py from the same
start.  Default: about 1e5 and 1e6 points per cloud.  Per size, one JSON row with
  mi_ndt_voxels and mi_voxel_downsample on the fixed cloud at the NDT voxel (whole call, host clock, median);
  for mi_ndt_register at 1 and 7 voxels per point and for mi_icp_gicp_register: the whole call (host clock, profiling off, median) and its
  stages with the stream drained after each (profiling on); ms per iteration of the step kernel and of the reduce-and-solve launches
  (profiling on, sync_every = 1; mi_profile_get books them under "nn" and "solve"); the iteration count, the stop reason and the distance
  from the ground truth.
    python tools/ndt_bench.py [--out FILE] [points ...]"""
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
from gicp_bench import EPSILON, K_NEIGHBOURS, timed  # noqa: E402
from plane_icp_bench import STAGES, VOXEL, median, pair  # noqa: E402

NDT_VOXEL = 10 * VOXEL
NDT_STAGES = ("workspace", "upload", "check", "table", "order", "iterations", "download", "total")


def registration(capi, ctx, G, register, params, times, stages):
    """register(params(**kw)) -> (R, t, iterations, error or score, stop): one method's figures"""
    (R, t, it, err, why), call = timed(lambda: register(params()))
    ctx.profile_enable(True)
    ctx.profile_reset()
    staged = {s: [] for s in stages}
    for _ in range(5):
        register(params(sync_every=1))
        now = times()
        for s in stages:
            staged[s].append(now[s])
    step_ms, step_n = ctx.profile_get(capi.KERNEL_NN)
    solve_ms, solve_n = ctx.profile_get(capi.KERNEL_SOLVE)
    ctx.profile_enable(False)
    ctx.profile_reset()
    return {"call_ms": round(median(call), 4), "call_ms_min": round(min(call), 4), "staged_ms": {s: round(median(v), 4) for s, v in staged.items()},
            "step_kernel_ms_per_iteration": round(step_ms / step_n, 5), "reduce_solve_ms_per_iteration": round(solve_ms / solve_n, 5),
            "launches_timed": [int(step_n), int(solve_n)], "iterations": it, "stop_reason": why, "error_or_score": float(err),
            "off_truth_dR_dt": [float(np.abs(R - G[:3, :3]).max()), float(np.abs(t - G[:3, 3]).max())]}


def one(capi, ctx, target):
    moving, fixed, _, G = pair(ctx, target)
    limit = (5 * VOXEL) ** 2
    vox, voxels_ms = timed(lambda: ctx.ndt_voxels(fixed, NDT_VOXEL), repeat=5, warm=1)
    _, downsample_ms = timed(lambda: ctx.voxel_downsample(fixed, NDT_VOXEL), repeat=5, warm=1)
    cov_a = ctx.estimate_covariances(fixed, K_NEIGHBOURS, capi.COV_PLANE, EPSILON)
    cov_b = ctx.estimate_covariances(moving, K_NEIGHBOURS, capi.COV_PLANE, EPSILON)
    row = {"target": target, "n_moving": len(moving), "m_fixed": len(fixed), "ndt_voxel": NDT_VOXEL, "voxels": len(vox["coord"]),
           "voxels_with_a_distribution": int((vox["icov"] != 0).any(axis=1).sum()),
           "ndt_voxels_call_ms": round(median(voxels_ms), 4), "voxel_downsample_call_ms": round(median(downsample_ms), 4)}
    for nb in (1, 7):
        row["ndt_%d" % nb] = registration(capi, ctx, G, lambda p: ctx.ndt_register(moving, vox, p), lambda **kw: capi.ndt_params(neighbourhood=nb, **kw),
                                          ctx.ndt_times, NDT_STAGES)
    row["gicp"] = registration(capi, ctx, G, lambda p: ctx.icp_gicp_register(moving, cov_b, fixed, cov_a, p),
                               lambda **kw: capi.plane_params(max_distance_squared=limit, **kw), ctx.icp_gicp_times, STAGES)
    for nb in (1, 7):
        row["step_kernel_ndt_%d_over_gicp" % nb] = round(row["ndt_%d" % nb]["step_kernel_ms_per_iteration"] / row["gicp"]["step_kernel_ms_per_iteration"], 3)
    return row


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
    doc = {"tool": "ndt_bench", "pair": "z = 0.3 sin(1.5 x) cos(1.2 y) + 2 mm noise, voxel 0.02; NDT map at voxel 0.2, min_points 6, eig_ratio 0.01, outlier ratio 0.55; "
                                        "GICP covariances MI_COV_PLANE epsilon 1e-3 k = 16, limit (5 voxels)^2; start 2 degrees and 0.02 off",
           "calls": "median of 7 whole calls after 2 warm-up calls; 5 staged and profiled calls per method", "rows": rows}
    print(json.dumps(doc), flush=True)
    if out:
        with open(out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
