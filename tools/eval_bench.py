#!/usr/bin/env python3
"""mi_evaluate_registration on tools/plane_icp_bench.py's scan-like pair (both clouds drawn from z = 0.3 sin(1.5 x) cos(1.2 y) plus 2 mm of
noise, voxel-filtered at 0.02, the fixed cloud's normals from k = 16), evaluated at the ground-truth pose under a limit of (5 voxels)^2.
Default: about 1e5 and 1e6 points per cloud.  Per size, one JSON row:
  the whole call in search mode and with the pairs given (search mode's own out_idx), host clock, profiling off, median of 7 after 2 warm-ups;
  the stages of both with the stream drained after each (mi_evaluate_registration_times, profiling on, median of 5);
  K55 alone in both modes (mi_profile_get books the step under "nn", the rows reduce under "solve"), beside K16's step in mi_plane_system and
  the search stage of mi_knn_search with k = 1 on the moved cloud, on the same clouds, pose and limit: the three are taken in turns, REPEATS
  times, so that what else the machine does falls on all alike; medians, the spread (min, max) of each, and the ratio K55 / K16.
    python tools/eval_bench.py [points ...]"""
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
from plane_icp_bench import VOXEL, median, pair  # noqa: E402

STAGES = ("workspace", "upload", "check", "grid", "order", "step", "download", "total")
REPEATS = 9


def spread(v):
    return {"median": round(median(v), 5), "min": round(min(v), 5), "max": round(max(v), 5)}


def whole_call(call):
    ms = []
    for i in range(2 + 7):
        t0 = time.perf_counter()
        call()
        if i >= 2:
            ms.append((time.perf_counter() - t0) * 1e3)
    return {"median": round(median(ms), 4), "min": round(min(ms), 4)}


def one(capi, ctx, target):
    moving, fixed, normals, G = pair(ctx, target)
    T = G.astype(np.float32)
    limit = (5 * VOXEL) ** 2
    fitness, rmse, info, idx = ctx.evaluate_registration(moving, fixed, T, max_d2=limit, want_idx=True)
    moved = (moving.astype(np.float64) @ G[:3, :3].T + G[:3, 3]).astype(np.float32)

    def search():
        return ctx.evaluate_registration(moving, fixed, T, max_d2=limit)

    def given():
        return ctx.evaluate_registration(moving, fixed, T, pairs=idx, max_d2=limit)

    calls = {"search": whole_call(search), "given": whole_call(given)}
    ctx.profile_enable(True)
    staged = {}
    for name, call in (("search", search), ("given", given)):
        rows = {s: [] for s in STAGES}
        for _ in range(5):
            call()
            times = ctx.evaluate_registration_times()
            for s in STAGES:
                rows[s].append(times[s])
        staged[name] = {s: round(median(v), 4) for s, v in rows.items()}

    def kernel(call):
        ctx.profile_reset()
        call()
        (step_ms, step_n), (sum_ms, sum_n) = ctx.profile_get(capi.KERNEL_NN), ctx.profile_get(capi.KERNEL_SOLVE)
        assert step_n == 1 and sum_n == 1
        return step_ms, sum_ms

    k55, k55_given, k16, reduce_ms, knn = [], [], [], [], []
    for _ in range(REPEATS):
        a = kernel(search)
        k55.append(a[0]); reduce_ms.append(a[1])
        k16.append(kernel(lambda: ctx.plane_system(moving, fixed, normals, T, max_d2=limit, want_idx=False))[0])
        k55_given.append(kernel(given)[0])
        ctx.knn_search(moved, fixed, 1, max_d2=limit, want_d2=False)
        knn.append(ctx.knn_search_times()["search"])
    ctx.profile_enable(False)
    ctx.profile_reset()
    return {"target": target, "n_moving": len(moving), "m_fixed": len(fixed), "fitness": fitness, "inlier_rmse": rmse,
            "call_ms": calls, "staged_ms": staged,
            "k55_search_ms": spread(k55), "k55_given_ms": spread(k55_given), "rows_reduce_ms": spread(reduce_ms),
            "k16_step_ms": spread(k16), "knn_k1_search_ms": spread(knn),
            "k55_over_k16": round(median(k55) / median(k16), 3), "k55_over_knn_search": round(median(k55) / median(knn), 3)}


def main():
    capi = load_package().capi
    sizes = [int(float(a)) for a in sys.argv[1:]] or [10 ** 5, 10 ** 6]
    rows = []
    with capi.Context(0) as ctx:
        ctx.preload()
        for target in sizes:
            rows.append(one(capi, ctx, target))
    print(json.dumps({"tool": "eval_bench", "pair": "z = 0.3 sin(1.5 x) cos(1.2 y) + 2 mm noise, voxel 0.02; the ground-truth pose; limit (5 voxels)^2",
                      "calls": "median of 7 whole calls after 2 warm-up calls; 5 staged calls per mode; kernels: %d rounds taken in turns" % REPEATS, "rows": rows}),
          flush=True)


if __name__ == "__main__":
    main()
