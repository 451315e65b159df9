#!/usr/bin/env python3
"""mi_tsdf_mesh on tools/tsdf_bench.py's synthetic room (10 x 8 x 3 units, voxel 0.05, S = 3) fused from 10 and from 100 scans of 1e5 points.
Per map: the whole call with both capacities known (host clock, profiling off: median, minimum, maximum) taken in turns with mi_tsdf_extract
of the same map, capacity known too -- the difference is the price of the triangles; then both calls' stages with the stream drained after
each (mi_tsdf_times, profiling on, median), the mesh's own launches (cases, used crossings, triangle fill: booked under "moments") and the
vertex fill it shares with the extraction (under "nn"), and vertices and triangles per second of the whole call.  One JSON line per map.
    python tools/tsdf_mesh_bench.py [--quick]"""
import ctypes as C
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
from tsdf_bench import KERNEL_MOMENTS, KERNEL_NN, VOXEL, room_scan, spread  # noqa: E402

WARM, CALLS, STAGED, S = 2, 9, 3, 3


def staged(ctx, run):
    ctx.profile_enable(True)
    ctx.profile_reset()
    stages = {}
    for _ in range(STAGED):
        run()
        for k, v in ctx.tsdf_times().items():
            stages.setdefault(k, []).append(v)
    nn, moments = ctx.profile_get(KERNEL_NN)[0] / STAGED, ctx.profile_get(KERNEL_MOMENTS)[0] / STAGED
    ctx.profile_enable(False)
    return {k: round(float(np.median(v)), 3) for k, v in stages.items()}, round(nn, 3), round(moments, 3)


def row(capi, ctx, rng, scans, points):
    clouds, poses = zip(*[room_scan(rng, points) for _ in range(scans)])
    origin = np.full(3, -1, np.float32)
    m = ctx.tsdf_integrate(clouds, np.array(poses), origin, capi.tsdf_params(voxel_size=VOXEL, truncation=S * VOXEL / 2 * 1.001))
    coord, tsdf, weight = (np.ascontiguousarray(a) for a in m)
    nv = len(tsdf)
    xyz, normals, tri = ctx.tsdf_mesh(m, origin, VOXEL)
    points_out = len(ctx.tsdf_extract(m, origin, VOXEL)[0])
    nvert, ntri = len(xyz), len(tri)
    surf, surf_n = np.empty((points_out, 3), np.float32), np.empty((points_out, 3), np.float32)
    a, b = C.c_longlong(0), C.c_longlong(0)
    head = (ctx._h, coord.ctypes.data, tsdf.ctypes.data, weight.ctypes.data, nv, origin.ctypes.data, float(VOXEL), 1.0)

    def mesh():
        rc = capi.tsdf_mesh_raw(*head, xyz.ctypes.data, normals.ctypes.data, nvert, C.addressof(a), tri.ctypes.data, ntri, C.addressof(b))
        assert rc == 0 and (a.value, b.value) == (nvert, ntri)

    def extract():
        rc = capi.tsdf_extract_raw(*head, surf.ctypes.data, surf_n.ctypes.data, points_out, C.addressof(a))
        assert rc == 0 and a.value == points_out

    ms = {"mesh": [], "extract": []}
    for i in range(WARM + CALLS):                        # in turns: whatever drifts, drifts under both
        for name, run in (("mesh", mesh), ("extract", extract)):
            t0 = time.perf_counter()
            run()
            if i >= WARM:
                ms[name].append((time.perf_counter() - t0) * 1e3)
    mesh_stages, mesh_nn, mesh_own = staged(ctx, mesh)
    extract_stages, extract_nn, _ = staged(ctx, extract)
    med = float(np.median(ms["mesh"]))
    return {"tool": "tsdf_mesh_bench", "scans": scans, "points_per_scan": points, "S": S, "voxels": nv, "vertices": nvert, "triangles": ntri,
            "extract_points": points_out,
            "mesh": {"call_ms": spread(ms["mesh"]), "staged_ms": mesh_stages, "cases_edges_triangles_kernels_ms": mesh_own, "vertex_fill_kernel_ms": mesh_nn,
                     "vertices_per_s": round(nvert / med * 1e3), "triangles_per_s": round(ntri / med * 1e3)},
            "extract": {"call_ms": spread(ms["extract"]), "staged_ms": extract_stages, "crossing_kernels_ms": extract_nn},
            "price_of_the_triangles_ms": round(med - float(np.median(ms["extract"])), 3),
            "calls": "%d whole calls of each in turns after %d warm-up, %d staged calls" % (CALLS, WARM, STAGED)}


def main():
    quick = "--quick" in sys.argv[1:]
    capi = load_package().capi
    rng = np.random.default_rng(0)
    with capi.Context(0) as ctx:
        for scans in ((10,) if quick else (10, 100)):
            print(json.dumps(row(capi, ctx, rng, scans, 100_000)), flush=True)


if __name__ == "__main__":
    main()
