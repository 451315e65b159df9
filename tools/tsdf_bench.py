#!/usr/bin/env python3
"""mi_tsdf_integrate and mi_tsdf_extract on a synthetic room (10 x 8 x 3 units, voxel 0.05): 10 and 100 posed scans of about 1e5 points, at
S = 3 and S = 6 half steps.  Per row: the whole integrate call with the capacity known (host clock, profiling off: median, minimum,
maximum), its stages with the stream drained after each (mi_tsdf_times, profiling on, median), the sampling launches (count and fill
together) and the fusion kernel alone (mi_profile_get books them under "nn" and "moments"), the same for the extraction of the fused map,
and mi_voxel_downsample on a cloud of as many points as there were samples: the same sort and segmented sums, so the difference is the
price of the rays.  One JSON line per row.
    python tools/tsdf_bench.py [--quick]"""
import ctypes as C
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

KERNEL_NN, KERNEL_MOMENTS = 0, 1      # MI_KERNEL_NN, MI_KERNEL_MOMENTS
WARM, CALLS, STAGED = 1, 5, 3
ROOM = np.array([10.0, 8.0, 3.0])
VOXEL = 0.05


def spread(v):
    v = np.asarray(v, np.float64)
    return {"median": round(float(np.median(v)), 3), "min": round(float(v.min()), 3), "max": round(float(v.max()), 3)}


def measure(ctx, run, times):
    """whole calls with profiling off, then staged calls with profiling on: (call spread, staged medians, ms per call under nn and moments)"""
    call = []
    for i in range(WARM + CALLS):
        t0 = time.perf_counter()
        run()
        if i >= WARM:
            call.append((time.perf_counter() - t0) * 1e3)
    ctx.profile_enable(True)
    ctx.profile_reset()
    staged = {}
    for _ in range(STAGED):
        run()
        for k, v in times().items():
            staged.setdefault(k, []).append(v)
    nn, moments = ctx.profile_get(KERNEL_NN)[0] / STAGED, ctx.profile_get(KERNEL_MOMENTS)[0] / STAGED
    ctx.profile_enable(False)
    return spread(call), {k: round(float(np.median(v)), 3) for k, v in staged.items()}, round(nn, 3), round(moments, 3)


def room_scan(rng, points):
    """a sensor somewhere in the room, turned about z; the walls, floor and ceiling it sees along `points` random directions, in its frame"""
    o = rng.uniform(0.2 * ROOM, 0.8 * ROOM)
    d = rng.normal(size=(points, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    with np.errstate(divide="ignore"):
        reach = np.where(d > 0, (ROOM - o) / d, np.where(d < 0, -o / d, np.inf)).min(axis=1)
    world = o + reach[:, None] * d + 0.005 * rng.normal(size=(points, 3))
    yaw = rng.uniform(0, 2 * np.pi)
    T = np.eye(4)
    T[:3, :3] = [[np.cos(yaw), -np.sin(yaw), 0], [np.sin(yaw), np.cos(yaw), 0], [0, 0, 1]]
    T[:3, 3] = o
    return ((world - o) @ T[:3, :3]).astype(np.float32), T


def row(capi, ctx, rng, scans, points, S):
    clouds, poses = zip(*[room_scan(rng, points) for _ in range(scans)])
    origin = np.full(3, -1, np.float32)
    params = capi.tsdf_params(voxel_size=VOXEL, truncation=S * VOXEL / 2 * 1.001)
    m = ctx.tsdf_integrate(clouds, np.array(poses), origin, params)
    nv, samples = len(m[0]), int(m[2].astype(np.float64).sum())
    xyz = np.ascontiguousarray(np.concatenate(clouds))
    offsets = (np.arange(scans + 1) * points).astype(np.int64)
    T = np.ascontiguousarray(np.array(poses).transpose(0, 2, 1), np.float32)
    out = (np.empty((nv, 3), np.int32), np.empty(nv, np.float32), np.empty(nv, np.float32))
    got = C.c_longlong(0)

    def integrate():
        rc = capi.tsdf_integrate_raw(ctx._h, xyz.ctypes.data, offsets.ctypes.data, scans, T.ctypes.data, origin.ctypes.data, C.addressof(params), None, None, None, 0,
                                     out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data, nv, C.addressof(got))
        assert rc == 0 and got.value == nv

    call, staged, nn, moments = measure(ctx, integrate, ctx.tsdf_times)
    res = {"tool": "tsdf_bench", "scans": scans, "points_per_scan": points, "S": S, "samples": samples, "voxels": nv,
           "integrate": {"call_ms": call, "staged_ms": staged, "sampling_kernels_ms": nn, "fusion_kernel_ms": moments}}
    surf = ctx.tsdf_extract(m, origin, VOXEL)[0]
    call, staged, nn, _ = measure(ctx, lambda: ctx.tsdf_extract(m, origin, VOXEL), ctx.tsdf_times)
    res["extract"] = {"points": len(surf), "call_ms_two_calls_inside": call, "staged_ms_of_the_filling_call": staged, "crossing_kernels_ms": nn}
    cloud = rng.random((samples, 3), dtype=np.float32) * ROOM.astype(np.float32)
    call, staged, _, _ = measure(ctx, lambda: ctx.voxel_downsample(cloud, VOXEL, origin=origin), ctx.voxel_downsample_times)
    res["voxel_downsample_of_as_many_points"] = {"call_ms": call, "staged_ms": staged}
    res["calls"] = "%d whole calls after %d warm-up, %d staged calls" % (CALLS, WARM, STAGED)
    return res


def main():
    quick = "--quick" in sys.argv[1:]
    capi = load_package().capi
    rng = np.random.default_rng(0)
    with capi.Context(0) as ctx:
        for scans in ((10,) if quick else (10, 100)):
            for S in (3, 6):
                print(json.dumps(row(capi, ctx, rng, scans, 100_000, S)), flush=True)


if __name__ == "__main__":
    main()
