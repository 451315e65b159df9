#!/usr/bin/env python3
"""mi_fgr_register beside mi_ransac_register on the same matches: C = 1e4 and 1e5 planted matches by default (unit cube, a rotation of
1 rad, noise 0.002, 40 % of the matches pointing at random places, delta = 0.02), FGR at its defaults (tuple filter 0.95, 1 000 tuples, 64
iterations) and without the filter (every match used once: the step's row count is C / 64), RANSAC at its default budget (1e5 hypotheses,
edge similarity 0.9, 2 refinement passes, max_distance = delta).  Per row: the whole call (host clock, profiling off, median and minimum
of 7 after 2 warm-up calls); the stages with the stream drained after each (mi_fgr_register_times / mi_ransac_register_times, profiling on,
median of 5); the step and the reduce-and-solve launches per iteration (profiling on, sync_every = 1; mi_profile_get books them under "nn"
and "solve"); the pose's distance from the planted one.  One JSON line; `--out FILE` keeps it.
    python tools/fgr_bench.py [--out FILE] [matches ...]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
for _v in ("OPENBLAS_NUM_THREADS", "OMP_NUM_THREADS", "MKL_NUM_THREADS"):   # see bench.quiet_host_pools: BLAS pools vs the CPU quota
    os.environ.setdefault(_v, "1")
import numpy as np  # noqa: E402
from __graft_entry__ import load_package  # noqa: E402
from fgr_reference import planted  # noqa: E402

DELTA, WARM, CALLS, STAGED = 0.02, 2, 7, 5


def median(v):
    return float(np.median(np.asarray(v, np.float64)))


def timed(call):
    ms = []
    for i in range(WARM + CALLS):
        t0 = time.perf_counter()
        out = call()
        if i >= WARM:
            ms.append((time.perf_counter() - t0) * 1e3)
    return out, ms


def fgr_row(capi, ctx, src, tgt, idx, R0, t0, **kw):
    out, ms = timed(lambda: ctx.fgr_register(src, tgt, idx, capi.fgr_params(DELTA, **kw)))
    R, t, it, err, why, used, mu = out
    ctx.profile_enable(True)
    ctx.profile_reset()
    staged = []
    for _ in range(STAGED):
        ctx.fgr_register(src, tgt, idx, capi.fgr_params(DELTA, sync_every=1, **kw))
        staged.append(ctx.fgr_register_times())
    step_ms, step_n = ctx.profile_get(capi.KERNEL_NN)
    solve_ms, solve_n = ctx.profile_get(capi.KERNEL_SOLVE)
    ctx.profile_enable(False)
    ctx.profile_reset()
    return {"call_ms": round(median(ms), 4), "call_ms_min": round(min(ms), 4), "staged_ms": {s: round(median([x[s] for x in staged]), 4) for s in staged[0]},
            "step_kernel_ms_per_iteration": round(step_ms / max(step_n, 1), 5), "reduce_solve_ms_per_iteration": round(solve_ms / max(solve_n, 1), 5),
            "launches_timed": [int(step_n), int(solve_n)], "used": int(used), "rows": (int(used) + 63) // 64, "iterations": int(it), "stop_reason": int(why),
            "final_mu": float(mu), "off_truth_dR_dt": [float(np.linalg.norm(R - R0)), float(np.linalg.norm(t - t0))]}


def ransac_row(capi, ctx, src, tgt, idx, R0, t0):
    p = capi.ransac_params(DELTA)
    out, ms = timed(lambda: ctx.ransac_register(src, tgt, idx, p))
    R, t, inl, rmse, best, nvalid = out
    ctx.profile_enable(True)
    staged = []
    for _ in range(STAGED):
        ctx.ransac_register(src, tgt, idx, p)
        staged.append(ctx.ransac_register_times())
    ctx.profile_enable(False)
    ctx.profile_reset()
    return {"call_ms": round(median(ms), 4), "call_ms_min": round(min(ms), 4), "staged_ms": {s: round(median([x[s] for x in staged]), 4) for s in staged[0]},
            "hypotheses": int(p.hypotheses), "valid_hypotheses": int(nvalid), "inliers": int(inl), "off_truth_dR_dt": [float(np.linalg.norm(R - R0)), float(np.linalg.norm(t - t0))]}


def main():
    args = sys.argv[1:]
    out_file = args.pop(args.index("--out") + 1) if "--out" in args else None
    args = [a for a in args if a != "--out"]
    capi = load_package().capi
    rows = []
    with capi.Context(0) as ctx:
        ctx.preload()
        for C in [int(float(a)) for a in args] or [10 ** 4, 10 ** 5]:
            src, tgt, idx, R0, t0, _ = planted(C, 0.4, 2026)
            rows.append({"matches": C, "fgr_default": fgr_row(capi, ctx, src, tgt, idx, R0, t0, seed=1), "fgr_no_filter": fgr_row(capi, ctx, src, tgt, idx, R0, t0, tuple_scale=0.0),
                         "ransac_default": ransac_row(capi, ctx, src, tgt, idx, R0, t0)})
    doc = {"tool": "fgr_bench", "pair": "unit cube, 1 rad, noise 0.002, 40 % wrong matches, delta 0.02", "calls": "median of %d whole calls after %d warm-up calls; %d staged and profiled calls" % (CALLS, WARM, STAGED), "rows": rows}
    line = json.dumps(doc)
    print(line)
    if out_file:
        with open(out_file, "w") as fh:
            fh.write(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
