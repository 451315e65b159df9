#!/usr/bin/env python3
"""mi_scan_context and mi_scan_context_search at their default shape (20 rings, 60 sectors).
Descriptors: 100 scans of about 1e5 points each in one call: the whole call (host clock, profiling off: median, minimum, maximum), its
stages with the stream drained after each (mi_scan_context_times, profiling on, median) and the binning kernel alone (mi_profile_get books
it under "moments").  Search: nd = 1e4 and 1e5 stored descriptors, nq = 1 and 100 queries: the whole call, the stages, the search launch
alone (mi_profile_get, "nn") and the rate that makes -- 2 nq nd sectors rings sectors floating-point operations, the padding to the
instruction's 64 x 2 KS x 64 not counted -- against the 157.3 TFLOP/s fp32 matrix peak of an MI355X.  Beside each search row,
mi_feature_match's search launch at about the same number of multiply-adds (n = nq sectors queries against m = nd sectors targets of dim =
rings, capped at the call's row limit: the row says what it ran), as the yardstick.  One JSON line per row.
    python tools/scan_context_bench.py [--quick]"""
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

PEAK_TFLOPS = 157.3
KERNEL_NN, KERNEL_MOMENTS = 0, 1      # MI_KERNEL_NN, MI_KERNEL_MOMENTS
WARM, CALLS, STAGED = 2, 7, 5


def spread(v):
    v = np.asarray(v, np.float64)
    return {"median": round(float(np.median(v)), 4), "min": round(float(v.min()), 4), "max": round(float(v.max()), 4)}


def measure(ctx, run, times, kernel):
    """whole calls with profiling off, then staged calls with profiling on: (call spread, staged medians, the kernel's ms per span)"""
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
    ms, spans = ctx.profile_get(kernel)
    ctx.profile_enable(False)
    return spread(call), {k: round(float(np.median(v)), 4) for k, v in staged.items() if not k.startswith("unused")}, ms / max(spans, 1)


def descriptor_row(capi, ctx, rng, scans, points):
    xyz = np.concatenate([rng.uniform(-90, 90, (scans * points, 2)), rng.uniform(-3, 12, (scans * points, 1))], axis=1).astype(np.float32)
    offsets = (np.arange(scans + 1) * points).astype(np.int32)
    params = capi.scan_context_params()
    call, staged, kernel_ms = measure(ctx, lambda: ctx.scan_context(xyz, offsets=offsets, params=params), ctx.scan_context_times, KERNEL_MOMENTS)
    return {"tool": "scan_context_bench", "call": "mi_scan_context", "scans": scans, "points_per_scan": points, "call_ms": call, "staged_ms": staged,
            "bins_kernel_ms": round(kernel_ms, 4), "points_per_ns_of_the_kernel": round(scans * points / (kernel_ms * 1e6), 2),
            "calls": "%d whole calls after %d warm-up calls, %d staged calls" % (CALLS, WARM, STAGED)}


def search_row(capi, ctx, rng, nq, nd):
    params = capi.scan_context_params()
    R, S = params.rings, params.sectors
    db = (rng.uniform(0, 12, (nd, R, S)) * (rng.uniform(0, 1, (nd, R, S)) < 0.6)).astype(np.float32)
    query = np.roll(db[rng.integers(0, nd, nq)], 11, axis=2) + rng.uniform(0, 0.2, (nq, R, S)).astype(np.float32)
    call, staged, kernel_ms = measure(ctx, lambda: ctx.scan_context_search(query, db, params=params), ctx.scan_context_times, KERNEL_NN)
    tflops = 2.0 * nq * nd * S * R * S / (kernel_ms * 1e9)
    row = {"tool": "scan_context_bench", "call": "mi_scan_context_search", "nq": nq, "nd": nd, "rings": R, "sectors": S, "call_ms": call,
           "staged_ms": staged, "search_kernel_ms": round(kernel_ms, 4), "tflops": round(tflops, 2),
           "fraction_of_fp32_matrix_peak": round(tflops / PEAK_TFLOPS, 4)}
    # the yardstick: mi_feature_match's search launch over about as many multiply-adds
    n, m = nq * S, min(nd * S, 4_000_000)
    q, t = rng.uniform(0, 1, (n, R)).astype(np.float32), rng.uniform(0, 1, (m, R)).astype(np.float32)
    _, _, match_ms = measure(ctx, lambda: ctx.feature_match(q, t), ctx.feature_match_times, KERNEL_NN)
    match_tflops = 2.0 * n * m * R / (match_ms * 1e9)
    row["feature_match"] = {"n": n, "m": m, "dim": R, "search_kernel_ms": round(match_ms, 4), "tflops": round(match_tflops, 2),
                            "fraction_of_fp32_matrix_peak": round(match_tflops / PEAK_TFLOPS, 4)}
    row["calls"] = "%d whole calls after %d warm-up calls, %d staged calls" % (CALLS, WARM, STAGED)
    return row


def main():
    quick = "--quick" in sys.argv[1:]
    capi = load_package().capi
    rng = np.random.default_rng(0)
    with capi.Context(0) as ctx:
        print(json.dumps(descriptor_row(capi, ctx, rng, 10 if quick else 100, 100_000)), flush=True)
        for nd in ((10_000,) if quick else (10_000, 100_000)):
            for nq in (1, 100):
                print(json.dumps(search_row(capi, ctx, rng, nq, nd)), flush=True)


if __name__ == "__main__":
    main()
