#!/usr/bin/env python3
"""mi_icp_color_register on a textured scan-like pair: both clouds drawn from the surface z = 0.3 sin(1.5 x) cos(1.2 y) (plus 2 mm of
noise) and passed through mi_voxel_downsample at a 0.02 voxel, every point's intensity the texture 0.5 + 0.2 sin(2 x) + 0.2 cos(1.7 y) at
its place, the fixed cloud's normals from mi_estimate_normals (k = 16, turned upwards) and its gradients from mi_estimate_color_gradients
(k = 16), the moving cloud 2 degrees and 0.02 off.  Default: about 1e5 and 1e6 points per cloud.  Per size, one JSON row:
  the whole call (host clock, profiling off, median) and its stages with the stream drained after each (mi_icp_color_times, profiling on);
  ms per iteration of the step kernel K49 and of the reduce-and-solve launches (profiling on, sync_every = 1 so that no launch is an empty
  one behind the stop; mi_profile_get books them under "nn" and "solve"), beside K16's step kernel from mi_icp_plane_register on the same
  clouds, measured the same way in the same run;
  the whole call of mi_estimate_color_gradients beside that of mi_estimate_normals at k = 16 on the fixed cloud (host clock, median);
  the iteration count and the distance from the ground truth, beside mi_icp_plane_register on the same pair.
    python tools/color_icp_bench.py [points ...]"""
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
LAMBDA = 0.968
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


def texture(p):
    p = np.asarray(p, np.float64)
    return (0.5 + 0.2 * np.sin(2.0 * p[:, 0]) + 0.2 * np.cos(1.7 * p[:, 1])).astype(np.float32)


def pair(ctx, target):
    """(moving, its intensities, fixed, normals, intensities, ground truth [4, 4]): about `target` points each after the voxel filter"""
    rng = np.random.default_rng(666)
    side = float(np.sqrt(target) * VOXEL)
    Rg = rodrigues(np.deg2rad(2.0) * np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0))
    tg = 0.02 * np.array([0.6, -0.48, 0.64])
    fixed = np.ascontiguousarray(ctx.voxel_downsample(draw(rng, side, 3 * target).astype(np.float32), VOXEL))
    raw = draw(rng, side, 3 * target)
    moving = np.ascontiguousarray(ctx.voxel_downsample(((raw - tg) @ Rg).astype(np.float32), VOXEL))   # G^-1 of a second draw of the same surface
    ib = texture(moving.astype(np.float64) @ Rg.T + tg)                                                 # the texture where the point truly lies
    normals = ctx.estimate_normals(fixed, 16, viewpoint=np.array([0, 0, 1e4], np.float32))
    G = np.eye(4)
    G[:3, :3], G[:3, 3] = Rg, tg
    return moving, ib, fixed, normals, texture(fixed), G


def timed(call, repeats=7, warm=2):
    out = []
    for i in range(warm + repeats):
        t0 = time.perf_counter()
        result = call()
        if i >= warm:
            out.append((time.perf_counter() - t0) * 1e3)
    return out, result


def profiled_steps(capi, ctx, call, times):
    """5 profiled calls -> (the stages' medians, ms per step launch, ms per reduce-and-solve iteration, the launches timed)"""
    staged = {s: [] for s in STAGES}
    ctx.profile_reset()
    for _ in range(5):
        call()
        got = times()
        for s in STAGES:
            staged[s].append(got[s])
    step_ms, step_n = ctx.profile_get(capi.KERNEL_NN)
    solve_ms, solve_n = ctx.profile_get(capi.KERNEL_SOLVE)
    return {s: round(median(v), 4) for s, v in staged.items()}, step_ms / step_n, solve_ms / solve_n, [int(step_n), int(solve_n)]


def one(capi, ctx, target):
    moving, ib, fixed, normals, ia, G = pair(ctx, target)
    limit = (5 * VOXEL) ** 2
    grad_ms, grad = timed(lambda: ctx.estimate_color_gradients(fixed, normals, ia, 16))
    normals_ms, _ = timed(lambda: ctx.estimate_normals(fixed, 16))
    p = capi.plane_params(max_distance_squared=limit)
    call, (R, t, it, err, why) = timed(lambda: ctx.icp_color_register(moving, ib, fixed, normals, ia, grad, p, LAMBDA))
    plane_call, (Rp, tp, itp, errp, whyp) = timed(lambda: ctx.icp_plane_register(moving, fixed, normals, p))
    ctx.profile_enable(True)
    p1 = capi.plane_params(max_distance_squared=limit, sync_every=1)
    staged, step, solve, launches = profiled_steps(capi, ctx, lambda: ctx.icp_color_register(moving, ib, fixed, normals, ia, grad, p1, LAMBDA), ctx.icp_color_times)
    _, plane_step, plane_solve, plane_launches = profiled_steps(capi, ctx, lambda: ctx.icp_plane_register(moving, fixed, normals, p1), ctx.icp_plane_times)
    ctx.profile_enable(False)
    ctx.profile_reset()

    def off(R_, t_):
        return [float(np.abs(R_ - G[:3, :3]).max()), float(np.abs(t_ - G[:3, 3]).max())]

    return {"target": target, "n_moving": len(moving), "m_fixed": len(fixed), "call_ms": round(median(call), 4), "call_ms_min": round(min(call), 4),
            "staged_ms": staged,
            "step_kernel_ms_per_iteration": round(step, 5), "reduce_solve_ms_per_iteration": round(solve, 5), "launches_timed": launches,
            "plane_step_kernel_ms_per_iteration": round(plane_step, 5), "plane_reduce_solve_ms_per_iteration": round(plane_solve, 5),
            "plane_launches_timed": plane_launches, "step_over_plane_step": round(step / plane_step, 3),
            "gradients_k16_call_ms": round(median(grad_ms), 4), "normals_k16_call_ms": round(median(normals_ms), 4),
            "gradients_over_normals": round(median(grad_ms) / median(normals_ms), 3),
            "iterations": it, "stop_reason": why, "error": float(err), "off_truth_dR_dt": off(R, t),
            "point_to_plane": {"call_ms": round(median(plane_call), 4), "iterations": itp, "stop_reason": whyp, "error": float(errp), "off_truth_dR_dt": off(Rp, tp)}}


def main():
    capi = load_package().capi
    sizes = [int(float(a)) for a in sys.argv[1:]] or [10 ** 5, 10 ** 6]
    rows = []
    with capi.Context(0) as ctx:
        ctx.preload()
        for target in sizes:
            rows.append(one(capi, ctx, target))
    print(json.dumps({"tool": "color_icp_bench",
                      "pair": "z = 0.3 sin(1.5 x) cos(1.2 y) + 2 mm noise, voxel 0.02, texture 0.5 + 0.2 sin(2 x) + 0.2 cos(1.7 y), normals and gradients k = 16; "
                              "start 2 degrees and 0.02 off; limit (5 voxels)^2; lambda_geometric 0.968",
                      "calls": "median of 7 whole calls after 2 warm-up calls; 5 staged and profiled calls of either method", "rows": rows}), flush=True)


if __name__ == "__main__":
    main()
