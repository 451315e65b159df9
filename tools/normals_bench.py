#!/usr/bin/env python3
"""mi_estimate_normals on the synthetic uniform cloud (bench.synth_cloud: [-5, 5]^3, seed 666), host buffer in, normals out, beside
mi_knn_search in self mode at the same k on the same cloud in the same process (idx only, want_d2=False).
Default: 1e5, 1e6 and 1e7 points with k = 8, 16, 32.  Per row, for either call: the whole call (host clock, profiling off, median) and
its stages with the stream drained after each (mi_estimate_normals_times / mi_knn_search_times, profiling on, median; the kernel stage
is the launch's own HIP-event time); then the fused kernel over the search kernel, the whole call over the whole call, and the bytes
either call brings back.  One JSON line, in the field conventions of tests/golden/voxel_measured.json.
    python tools/normals_bench.py [points ...]"""
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

KNN_STAGES = ("workspace", "upload", "check", "grid", "order", "search", "download", "total")
NORMALS_STAGES = ("workspace", "upload", "check", "grid", "order", "fused", "download", "total")


def median(v):
    return float(np.median(np.asarray(v, np.float64)))


def repeats(n):
    """(warm-up, timed whole calls, staged calls): at least five of each kind, warm-up aside"""
    return (1, 5, 5) if n >= 5 * 10 ** 6 else (2, 7, 5)


def measure(capi, ctx, run, times, stages, n):
    """run() is one whole call returning the error code: (median and minimum of the whole call, staged medians)"""
    warm, calls, staged_calls = repeats(n)
    call = []
    for i in range(warm + calls):
        t0 = time.perf_counter()
        rc = run()
        if i >= warm:
            call.append((time.perf_counter() - t0) * 1e3)
        assert rc == capi.MI_OK, capi.lib().mi_last_error()
    ctx.profile_enable(True)
    staged = {s: [] for s in stages}
    for _ in range(staged_calls):
        rc = run()
        assert rc == capi.MI_OK, capi.lib().mi_last_error()
        t = times()
        for s in stages:
            staged[s].append(t[s])
    ctx.profile_enable(False)
    return round(median(call), 4), round(min(call), 4), {s: round(median(v), 4) for s, v in staged.items()}


def one(capi, ctx, cloud, k):
    n = len(cloud)
    inf = float("inf")
    idx = np.empty((n, k), np.int32)
    knn = measure(capi, ctx, lambda: capi.knn_search_raw(ctx._h, None, n, cloud.ctypes.data, n, k, capi.DIST_CPU_ROUNDING, inf, idx.ctypes.data, None, None),
                  ctx.knn_search_times, KNN_STAGES, n)
    del idx
    normals, curvature = np.empty((n, 3), np.float32), np.empty(n, np.float32)
    nrm = measure(capi, ctx, lambda: capi.estimate_normals_raw(ctx._h, cloud.ctypes.data, n, k, capi.DIST_CPU_ROUNDING, inf, None, normals.ctypes.data,
                                                              curvature.ctypes.data, None),
                  ctx.estimate_normals_times, NORMALS_STAGES, n)
    assert np.isfinite(normals).all() and np.abs(np.linalg.norm(normals[::997].astype(np.float64), axis=1) - 1).max() <= 2e-7
    return {"n": n, "k": k, "call_ms": nrm[0], "call_ms_min": nrm[1], "staged_ms": nrm[2], "fused_ns_per_point": round(nrm[2]["fused"] * 1e6 / n, 3),
            "download_bytes": 16 * n,
            "knn_call_ms": knn[0], "knn_call_ms_min": knn[1], "knn_staged_ms": knn[2], "knn_search_ns_per_point": round(knn[2]["search"] * 1e6 / n, 3),
            "knn_download_bytes": 4 * k * n,
            "fused_over_knn_search": round(nrm[2]["fused"] / knn[2]["search"], 3), "call_over_knn_call": round(nrm[0] / knn[0], 3)}


def main():
    capi = load_package().capi
    sizes = [int(float(a)) for a in sys.argv[1:]] or [10 ** 5, 10 ** 6, 10 ** 7]
    rows = []
    with capi.Context(0) as ctx:
        ctx.preload()
        for n in sizes:
            cloud = np.ascontiguousarray(synth_cloud(np, n)[0])
            for k in (8, 16, 32):
                rows.append(one(capi, ctx, cloud, k))
    print(json.dumps({"tool": "normals_bench", "cloud": "uniform [-5,5]^3, seed 666, self mode; normals + curvature out, idx out for the k-NN call",
                      "calls": "median of 7 whole calls after 2 warm-up calls and of 5 staged calls (1e7 points: 5 after 1, and 5)", "rows": rows}), flush=True)


if __name__ == "__main__":
    main()
