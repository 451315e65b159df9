#!/usr/bin/env python3
"""mi_fpfh_features on a scan-like cloud: points drawn from the surface z = 0.3 sin(1.5 x) cos(1.2 y) (plus 2 mm of noise), passed through
mi_voxel_downsample at a 0.02 voxel, with normals from mi_estimate_normals (k = 16, turned upwards) -- the cloud of tools/plane_icp_bench.py --
beside mi_estimate_normals at the same k on the same cloud in the same process: that call does the same search and less arithmetic behind
it, so it is the floor.  Default: about 1e5, 1e6 and 1e7 points with k = 8, 16, 32.  Per row, for either call: the whole call (host
clock, profiling off, median) and its stages with the stream drained after each (mi_fpfh_features_times / mi_estimate_normals_times,
profiling on, median; the kernel stage is the launches' own HIP-event time); the SPFH kernel (K18) and the FPFH kernel (K19) on their
own (profiling on; mi_profile_get books them under "nn" and "moments"); then K18 over the normals' fused kernel, what K19 gathers
(n k 40 bytes) and the rate that makes, and the whole call over the whole call.  One JSON line.
    python tools/fpfh_bench.py [points ...]"""
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
FPFH_STAGES = ("workspace", "upload", "check", "grid", "order", "kernels", "download", "total")
NORMALS_STAGES = ("workspace", "upload", "check", "grid", "order", "fused", "download", "total")
KERNEL_NN, KERNEL_MOMENTS = 0, 1      # MI_KERNEL_NN, MI_KERNEL_MOMENTS


def median(v):
    return float(np.median(np.asarray(v, np.float64)))


def surface(ctx, target):
    """(cloud, normals): about `target` points after the voxel filter"""
    rng = np.random.default_rng(666)
    side = float(np.sqrt(target) * VOXEL)
    xy = rng.uniform(-side / 2, side / 2, (3 * target, 2))
    z = 0.3 * np.sin(1.5 * xy[:, 0]) * np.cos(1.2 * xy[:, 1]) + rng.normal(0, 0.002, 3 * target)
    cloud = np.ascontiguousarray(ctx.voxel_downsample(np.concatenate([xy, z[:, None]], axis=1).astype(np.float32), VOXEL))
    return cloud, np.ascontiguousarray(ctx.estimate_normals(cloud, 16, viewpoint=np.array([0, 0, 1e4], np.float32)))


def repeats(n):
    """(warm-up, timed whole calls, staged calls): at least five of each kind, warm-up aside"""
    return (1, 5, 5) if n >= 5 * 10 ** 6 else (2, 7, 5)


def measure(capi, ctx, run, times, stages, n, kernels=()):
    """run() is one whole call returning the error code: (median and minimum of the whole call, staged medians, ms per launch of `kernels`)"""
    warm, calls, staged_calls = repeats(n)
    call = []
    for i in range(warm + calls):
        t0 = time.perf_counter()
        rc = run()
        if i >= warm:
            call.append((time.perf_counter() - t0) * 1e3)
        assert rc == capi.MI_OK, capi.lib().mi_last_error()
    ctx.profile_enable(True)
    ctx.profile_reset()
    staged = {s: [] for s in stages}
    for _ in range(staged_calls):
        rc = run()
        assert rc == capi.MI_OK, capi.lib().mi_last_error()
        t = times()
        for s in stages:
            staged[s].append(t[s])
    per_launch = []
    for kernel in kernels:
        ms, launches = ctx.profile_get(kernel)
        per_launch.append(round(ms / max(launches, 1), 4))
    ctx.profile_enable(False)
    return round(median(call), 4), round(min(call), 4), {s: round(median(v), 4) for s, v in staged.items()}, per_launch


def one(capi, ctx, cloud, normals_in, k):
    n = len(cloud)
    inf = float("inf")
    fpfh = np.empty((n, 33), np.float32)
    f = measure(capi, ctx, lambda: capi.fpfh_features_raw(ctx._h, cloud.ctypes.data, normals_in.ctypes.data, n, k, capi.DIST_CPU_ROUNDING, inf, fpfh.ctypes.data, None, None),
                ctx.fpfh_features_times, FPFH_STAGES, n, (KERNEL_NN, KERNEL_MOMENTS))
    sums = fpfh[::997].astype(np.float64).reshape(-1, 3, 11).sum(axis=2)
    assert np.isfinite(fpfh).all() and np.abs(sums - 200.0).max() <= 200.0 * 2.0 ** -23
    del fpfh
    normals, curvature = np.empty((n, 3), np.float32), np.empty(n, np.float32)
    nrm = measure(capi, ctx, lambda: capi.estimate_normals_raw(ctx._h, cloud.ctypes.data, n, k, capi.DIST_CPU_ROUNDING, inf, None, normals.ctypes.data,
                                                              curvature.ctypes.data, None),
                  ctx.estimate_normals_times, NORMALS_STAGES, n)
    spfh_ms, sum_ms = f[3]
    return {"n": n, "k": k, "call_ms": f[0], "call_ms_min": f[1], "staged_ms": f[2], "spfh_kernel_ms": spfh_ms, "fpfh_kernel_ms": sum_ms,
            "spfh_ns_per_point": round(spfh_ms * 1e6 / n, 3), "fpfh_ns_per_point": round(sum_ms * 1e6 / n, 3),
            "fpfh_gather_bytes": 40 * k * n, "fpfh_gather_gb_per_s": round(40.0 * k * n / (sum_ms * 1e6), 2), "download_bytes": 132 * n,
            "normals_call_ms": nrm[0], "normals_call_ms_min": nrm[1], "normals_staged_ms": nrm[2],
            "normals_fused_ns_per_point": round(nrm[2]["fused"] * 1e6 / n, 3),
            "spfh_over_normals_fused": round(spfh_ms / nrm[2]["fused"], 3), "kernels_over_normals_fused": round(f[2]["kernels"] / nrm[2]["fused"], 3),
            "call_over_normals_call": round(f[0] / nrm[0], 3)}


def main():
    capi = load_package().capi
    sizes = [int(float(a)) for a in sys.argv[1:]] or [10 ** 5, 10 ** 6, 10 ** 7]
    rows = []
    with capi.Context(0) as ctx:
        ctx.preload()
        for target in sizes:
            cloud, normals = surface(ctx, target)
            for k in (8, 16, 32):
                rows.append(one(capi, ctx, cloud, normals, k))
    print(json.dumps({"tool": "fpfh_bench", "cloud": "z = 0.3 sin(1.5 x) cos(1.2 y) + 2 mm noise, voxel 0.02, normals from k = 16; fpfh out; normals + curvature out for the normals call",
                      "calls": "median of 7 whole calls after 2 warm-up calls and of 5 staged calls (5e6 points and more: 5 after 1, and 5)", "rows": rows}), flush=True)


if __name__ == "__main__":
    main()
