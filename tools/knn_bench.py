#!/usr/bin/env python3
"""mi_knn_search on the synthetic uniform cloud (bench.synth_cloud: [-5, 5]^3, seed 666), host buffers in, idx and d2 out.
Default: self mode at 1e5, 1e6 and 1e7 points with k = 1, 8, 16, 32, and one row with separate queries (n = m = 1e6, k = 8).  Per row:
the whole call (host clock, profiling off, median), its stages with the stream drained after each (mi_knn_search_times, profiling on,
median; the search stage is the launch's own HIP-event time), search time per query, the compulsory bytes of the search over its time,
and the ratio to the yardstick measured in the same process: the plain cell-grid 1-NN search kernel on the same cloud as its own
query set (mi_nn_search_ex(..., MI_NN_GRID), kernel time from mi_profile_get(MI_KERNEL_NN)).
--sweep: at 1e6 points, k = 8 and k = 32, the search stage over MISLAM_KNN_POINTS_PER_CELL (a fresh context per value).  One JSON line.
    python tools/knn_bench.py [--sweep] [points ...]"""
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

STAGES = ("workspace", "upload", "check", "grid", "order", "search", "download", "total")
SWEEP = {8: (1.0, 2.0, 3.0, 4.0, 6.0, 8.0, 12.0), 32: (4.0, 8.0, 12.0, 16.0, 24.0, 32.0, 48.0)}


def median(v):
    return float(np.median(np.asarray(v, np.float64)))


def repeats(n):
    """(warm-up, timed whole calls, staged calls): fewer at 1e7 points, where a call moves gigabytes of results"""
    return (1, 3, 3) if n >= 5 * 10 ** 6 else (2, 7, 5)


def yardstick(capi, ctx, cloud):
    """ms of the cell-grid 1-NN search kernel, the cloud against itself (every query's answer is its own point)"""
    warm, _, staged = repeats(len(cloud))
    got = []
    for i in range(warm + staged):
        ctx.profile_enable(True)
        ctx.profile_reset()
        ctx.nn_search(cloud, cloud, capi.DIST_CPU_ROUNDING, capi.NN_GRID)
        ms, launches = ctx.profile_get(capi.KERNEL_NN)
        ctx.profile_enable(False)
        assert launches == 1
        if i >= warm:
            got.append(ms)
    return median(got)


def staged_search(capi, ctx, query, cloud, k, calls):
    n, m = (len(cloud) if query is None else len(query)), len(cloud)
    idx, d2 = np.empty((n, k), np.int32), np.empty((n, k), np.float32)
    qp = None if query is None else query.ctypes.data
    ctx.profile_enable(True)
    staged = {s: [] for s in STAGES}
    for _ in range(calls):
        rc = capi.knn_search_raw(ctx._h, qp, n, cloud.ctypes.data, m, k, capi.DIST_CPU_ROUNDING, float("inf"), idx.ctypes.data, d2.ctypes.data, None)
        assert rc == capi.MI_OK, capi.lib().mi_last_error()
        t = ctx.knn_search_times()
        for s in STAGES:
            staged[s].append(t[s])
    ctx.profile_enable(False)
    return {s: round(median(v), 4) for s, v in staged.items()}


def one(capi, ctx, query, cloud, k, yard_ms):
    n, m = (len(cloud) if query is None else len(query)), len(cloud)
    warm, calls, staged_calls = repeats(max(n, m))
    idx, d2 = np.empty((n, k), np.int32), np.empty((n, k), np.float32)
    qp = None if query is None else query.ctypes.data
    call = []
    for i in range(warm + calls):
        t0 = time.perf_counter()
        rc = capi.knn_search_raw(ctx._h, qp, n, cloud.ctypes.data, m, k, capi.DIST_CPU_ROUNDING, float("inf"), idx.ctypes.data, d2.ctypes.data, None)
        if i >= warm:
            call.append((time.perf_counter() - t0) * 1e3)
        assert rc == capi.MI_OK, capi.lib().mi_last_error()
    del idx, d2
    st = staged_search(capi, ctx, query, cloud, k, staged_calls)
    # what the search cannot avoid moving: a query and its order word in, k (idx, d2) pairs out, every sorted point once
    compulsory = n * 16 + n * k * 8 + m * 16
    return {"mode": "self" if query is None else "queries", "n": n, "m": m, "k": k, "call_ms": round(median(call), 4), "call_ms_min": round(min(call), 4),
            "staged_ms": st, "search_ns_per_query": round(st["search"] * 1e6 / n, 3), "yardstick_nn_grid_kernel_ms": round(yard_ms, 4),
            "yardstick_ns_per_query": round(yard_ms * 1e6 / m, 3), "search_over_yardstick": round(st["search"] / yard_ms * (m / n), 3),
            "search_compulsory_bytes": compulsory, "search_compulsory_GBps": round(compulsory / (st["search"] * 1e-3) / 1e9, 1)}


def sweep(capi, n):
    cloud = np.ascontiguousarray(synth_cloud(np, n)[0])
    rows = []
    for k, values in SWEEP.items():
        for ppc in values:
            os.environ["MISLAM_KNN_POINTS_PER_CELL"] = repr(ppc)          # read when the context is created
            with capi.Context(0) as ctx:
                st = staged_search(capi, ctx, None, cloud, k, 1 + 3)
            rows.append({"n": n, "k": k, "points_per_cell": ppc, "search_ms": st["search"], "grid_ms": st["grid"]})
    os.environ.pop("MISLAM_KNN_POINTS_PER_CELL", None)
    return rows


def main():
    capi = load_package().capi
    args = sys.argv[1:]
    do_sweep = "--sweep" in args
    sizes = [int(float(a)) for a in args if a != "--sweep"]
    if do_sweep:
        print(json.dumps({"tool": "knn_bench", "what": "sweep", "cloud": "uniform [-5,5]^3, seed 666, self mode", "rows": sweep(capi, (sizes or [10 ** 6])[0])}), flush=True)
        return
    rows = []
    with capi.Context(0) as ctx:
        ctx.preload()
        for n in sizes or [10 ** 5, 10 ** 6, 10 ** 7]:
            cloud = np.ascontiguousarray(synth_cloud(np, n)[0])
            yard = yardstick(capi, ctx, cloud)
            for k in (1, 8, 16, 32):
                rows.append(one(capi, ctx, None, cloud, k, yard))
            if n == 10 ** 6:
                query = np.ascontiguousarray(synth_cloud(np, n, seed=667)[0])
                rows.append(one(capi, ctx, query, cloud, 8, yard))
    print(json.dumps({"tool": "knn_bench", "what": "sizes", "cloud": "uniform [-5,5]^3, seed 666", "rows": rows}), flush=True)


if __name__ == "__main__":
    main()
