#!/usr/bin/env python3
"""mi_tsdf_raycast on tsdf_bench.py's synthetic room (10 x 8 x 3 units, voxel 0.05, S = 3), fused from 10 and 100 posed scans of about 1e5
points: a 640 x 480 pinhole view and a 64 x 1024 spherical sweep from the middle of the room, range 12 (K = 481 samples per ray).  Per row:
the whole call (host clock, profiling off: median, minimum, maximum), its stages with the stream drained after each (mi_tsdf_times,
profiling on, median: table, block table, cast), the cast kernel alone (mi_profile_get books it under "nn") with empty-space skipping and
with every sample visited, the two marches' outputs compared bit for bit, hits per second of the whole call, and beside them mi_tsdf_extract
of the same map (two calls inside) with its points per second.  One JSON line per row.
    python tools/tsdf_raycast_bench.py [--quick]"""
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
from tsdf_bench import ROOM, VOXEL, measure, room_scan  # noqa: E402

MAX_RANGE = 12.0


def views(capi):
    # the camera looks along the sensor's +x: its z ahead, its x to the sensor's -y, its y (down) to the sensor's -z
    mount = np.array([[0.0, -1.0, 0.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0]])
    pin = (capi.pinhole_directions(640, 480, 400.0, 400.0, 319.5, 239.5).astype(np.float64) @ mount).astype(np.float32)
    return {"pinhole_640x480": pin, "spherical_64x1024": capi.spherical_directions(64, 1024, -0.4, 0.4)}


def row(capi, ctx, rng, scans, points):
    clouds, poses = zip(*[room_scan(rng, points) for _ in range(scans)])
    origin = np.full(3, -1, np.float32)
    m = ctx.tsdf_integrate(clouds, np.array(poses), origin, capi.tsdf_params(voxel_size=VOXEL, truncation=3 * VOXEL / 2 * 1.001))
    nv = len(m[0])
    pose = np.eye(4)
    pose[:3, :3] = [[np.cos(0.3), -np.sin(0.3), 0], [np.sin(0.3), np.cos(0.3), 0], [0, 0, 1]]
    pose[:3, 3] = 0.5 * ROOM
    T = np.ascontiguousarray(pose.T, np.float32)
    res = {"tool": "tsdf_raycast_bench", "scans": scans, "points_per_scan": points, "voxels": nv, "samples_per_ray": int(MAX_RANGE / (VOXEL / 2)) + 1}
    for name, dirs in views(capi).items():
        n = len(dirs)
        out = (np.empty(n, np.float32), np.empty((n, 3), np.float32), np.empty((n, 3), np.float32))
        hits = C.c_longlong(0)
        kept = {}
        for label, visit in (("skipping", 0), ("every_sample", 1)):
            params = capi.tsdf_raycast_params(voxel_size=VOXEL, max_range=MAX_RANGE, visit_every_sample=visit)

            def cast():
                rc = capi.tsdf_raycast_raw(ctx._h, m[0].ctypes.data, m[1].ctypes.data, m[2].ctypes.data, nv, origin.ctypes.data, C.addressof(params),
                                           T.ctypes.data, dirs.ctypes.data, n, out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data, C.addressof(hits))
                assert rc == 0, capi.lib().mi_last_error().decode()

            call, staged, nn, _ = measure(ctx, cast, ctx.tsdf_times)
            kept[label] = [a.copy() for a in out] + [hits.value]
            res.setdefault(name, {"rays": n})[label] = {"call_ms": call, "staged_ms": staged, "cast_kernel_ms": nn, "hits": hits.value,
                                                        "hits_per_second_of_the_call": round(hits.value / (call["median"] * 1e-3))}
        a, b = kept["skipping"], kept["every_sample"]
        res[name]["the_two_marches_agree_bit_for_bit"] = bool(a[3] == b[3] and all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a[:3], b[:3])))
    surf = ctx.tsdf_extract(m, origin, VOXEL)[0]
    call, staged, nn, _ = measure(ctx, lambda: ctx.tsdf_extract(m, origin, VOXEL), ctx.tsdf_times)
    res["extract"] = {"points": len(surf), "call_ms_two_calls_inside": call, "crossing_kernels_ms": nn, "points_per_second_of_the_call": round(len(surf) / (call["median"] * 1e-3))}
    return res


def main():
    quick = "--quick" in sys.argv[1:]
    capi = load_package().capi
    rng = np.random.default_rng(0)
    with capi.Context(0) as ctx:
        for scans in ((10,) if quick else (10, 100)):
            print(json.dumps(row(capi, ctx, rng, scans, 100_000)), flush=True)


if __name__ == "__main__":
    main()
