#!/usr/bin/env python3
"""mi_voxel_downsample on the synthetic uniform cloud (bench.synth_cloud: [-5, 5]^3, seed 666) at 1e5, 1e6 and 1e7 points and two voxel
sizes -- about 8 points per voxel and about 1 -- host buffer in, rows out.  Per (n, voxel): the whole call (host clock, profiling off,
median), its stages with the stream drained after each (mi_voxel_downsample_times, profiling on, median) and, in the same process and
at the same n, the yardstick: the ordering stage of mi_icp_load (mi_icp_load_times stage 2, profiling on) -- the same radix sort over n
30-bit keys plus a permute.  One JSON line.
    python tools/voxel_bench.py [points ...]"""
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
from bench import synth_cloud  # noqa: E402

WARMUP, CALLS, STAGED = 2, 7, 5
STAGES = ("workspace", "upload", "range", "sort", "sums", "download", "total")


def median(v):
    return float(np.median(np.asarray(v, np.float64)))


def yardstick(capi, ctx, cloud):
    """ms of mi_icp_load's moving-cloud ordering stage at len(cloud) points (the fixed cloud is a handful of points, searched every-pair:
    no index build rides along)"""
    params = capi.icp_params(nn_mode=capi.NN_BRUTEFORCE)
    ctx.profile_enable(True)
    got = []
    for k in range(WARMUP + STAGED):
        ctx.icp_load(cloud, cloud[:1000], params)
        if k >= WARMUP:
            got.append(ctx.icp_load_times()["order_moving"])
    ctx.profile_enable(False)
    return median(got)


def one(capi, ctx, cloud, voxel, order_ms):
    n = len(cloud)
    for _ in range(WARMUP):
        rows = len(ctx.voxel_downsample(cloud, voxel))
    # the binding allocates the (n, 3) output array per call; the library call alone is timed
    out, got = np.empty((n, 3), np.float32), capi.C.c_int(0)
    call = []
    for _ in range(CALLS):
        t0 = time.perf_counter()
        rc = capi.voxel_downsample_raw(ctx._h, cloud.ctypes.data, n, float(voxel), None, out.ctypes.data, capi.C.addressof(got), None, None, None)
        call.append((time.perf_counter() - t0) * 1e3)
        assert rc == capi.MI_OK and got.value == rows
    ctx.profile_enable(True)
    staged = {k: [] for k in STAGES}
    for _ in range(STAGED):
        rc = capi.voxel_downsample_raw(ctx._h, cloud.ctypes.data, n, float(voxel), None, out.ctypes.data, capi.C.addressof(got), None, None, None)
        assert rc == capi.MI_OK
        t = ctx.voxel_downsample_times()
        for k in STAGES:
            staged[k].append(t[k])
    ctx.profile_enable(False)
    st = {k: round(median(v), 4) for k, v in staged.items()}
    device_side = st["range"] + st["sort"] + st["sums"]
    minus_upload = st["total"] - st["upload"] - st["workspace"]
    return {"n": n, "voxel": round(float(voxel), 6), "points_per_voxel_nominal": round(n * voxel ** 3 / 1000.0, 3), "rows": rows,
            "points_per_row": round(n / rows, 3), "call_ms": round(median(call), 4), "call_ms_min": round(min(call), 4), "staged_ms": st,
            "range_sort_sums_ms": round(device_side, 4), "call_minus_upload_ms": round(minus_upload, 4),
            "yardstick_icp_load_order_ms": round(order_ms, 4), "range_sort_sums_over_yardstick": round(device_side / order_ms, 3),
            "call_minus_upload_over_yardstick": round(minus_upload / order_ms, 3)}


def main():
    capi = load_package().capi
    sizes = [int(float(a)) for a in sys.argv[1:]] or [10 ** 5, 10 ** 6, 10 ** 7]
    rows = []
    with capi.Context(0) as ctx:
        ctx.preload()
        for n in sizes:
            cloud = np.ascontiguousarray(synth_cloud(np, n)[0])
            order_ms = yardstick(capi, ctx, cloud)
            for per_voxel in (8.0, 1.0):
                rows.append(one(capi, ctx, cloud, (1000.0 * per_voxel / n) ** (1.0 / 3.0), order_ms))
    print(json.dumps({"tool": "voxel_bench", "cloud": "uniform [-5,5]^3, seed 666", "warmup": WARMUP, "calls": CALLS, "staged_calls": STAGED,
                      "rows": rows}), flush=True)


if __name__ == "__main__":
    main()
