#!/usr/bin/env python3
"""mi_feature_match on descriptor-like rows: uniform [0, 200) rows of dim 33 (FPFH's range and size), n = m = 1e4 and 1e5 by default, with
and without the mutual filter.  Per row: the whole call (host clock, profiling off, median and minimum); its stages with the stream
drained after each (mi_feature_match_times, profiling on, median); the search launches alone (profiling on; mi_profile_get books them under
"nn": one launch per direction, both inside one span); and the rate that makes: 2 n m dim floating-point operations per direction (the
padding to the instruction's K and the keys are not counted) against the 157.3 TFLOP/s fp32 matrix peak of an MI355X.  One JSON line per
row.  Then mi_ransac_register at the same sizes as hypotheses and as matches (30 % true matches under a planted pose, max_distance 0.01,
edge similarity 0.9, 2 refinement passes): whole call, stages (mi_ransac_register_times), pair tests per ns of the counting kernel.  Then the three calls of a global registration on the same clouds (a bumpy closed surface
with analytic normals and a moved copy): mi_fpfh_features (k = 16), mi_feature_match (mutual), mi_ransac_register (1e5 hypotheses), at 3 000, 10 000 and 30 000 points.
    python tools/global_bench.py [rows ...]"""
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

DIM = 33
PEAK_TFLOPS = 157.3
STAGES = ("workspace", "upload", "check", "kernels", "download", "total")
KERNEL_NN = 0                         # MI_KERNEL_NN
WARM, CALLS, STAGED = 2, 7, 5


def median(v):
    return float(np.median(np.asarray(v, np.float64)))


def one(capi, ctx, q, t, mutual):
    n, m = len(q), len(t)
    idx, d2 = np.empty(n, np.int32), np.empty(n, np.float32)
    run = lambda: capi.feature_match_raw(ctx._h, q.ctypes.data, n, t.ctypes.data, m, DIM, mutual, idx.ctypes.data, d2.ctypes.data)
    call = []
    for i in range(WARM + CALLS):
        t0 = time.perf_counter()
        rc = run()
        if i >= WARM:
            call.append((time.perf_counter() - t0) * 1e3)
        assert rc == capi.MI_OK, capi.lib().mi_last_error()
    ctx.profile_enable(True)
    ctx.profile_reset()
    staged = {s: [] for s in STAGES}
    for _ in range(STAGED):
        rc = run()
        assert rc == capi.MI_OK, capi.lib().mi_last_error()
        ms = ctx.feature_match_times()
        for s in STAGES:
            staged[s].append(ms[s])
    search_ms, spans = ctx.profile_get(KERNEL_NN)
    ctx.profile_enable(False)
    search_ms /= max(spans, 1)
    # a sample of the answers against float64: the chosen target is the nearest within the key's rounding, a few ulp of |q|^2 + |t|^2
    for i in range(0, n, max(1, n // 16)):
        if idx[i] >= 0:
            exact = ((t.astype(np.float64) - q[i].astype(np.float64)) ** 2).sum(axis=1)
            assert exact[idx[i]] - exact.min() <= 64 * 2.0 ** -23 * 2 * DIM * 200.0 ** 2, i
    flop = 2.0 * n * m * DIM * (2 if mutual else 1)
    tflops = flop / (search_ms * 1e9)
    return {"tool": "global_bench", "call": "mi_feature_match", "n": n, "m": m, "dim": DIM, "mutual": mutual, "kept": int((idx >= 0).sum()),
            "call_ms": round(median(call), 4), "call_ms_min": round(min(call), 4), "staged_ms": {s: round(median(v), 4) for s, v in staged.items()},
            "search_kernels_ms": round(search_ms, 4), "tflops": round(tflops, 2), "fraction_of_fp32_matrix_peak": round(tflops / PEAK_TFLOPS, 4),
            "calls": "median of %d whole calls after %d warm-up calls and of %d staged calls" % (CALLS, WARM, STAGED)}


def planted(rng, C):
    """C matches, 30 % of them true under a 100 degree rotation with 1e-3 noise, the rest random: (src, tgt, idx)"""
    src = rng.uniform(-1, 1, (C, 3)).astype(np.float32)
    a = np.deg2rad(100.0)
    R0 = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    tgt = (src @ R0.T + [0.5, -1.0, 2.0] + 1e-3 * rng.uniform(-1, 1, (C, 3)) / np.sqrt(3)).astype(np.float32)
    idx = np.arange(C, dtype=np.int32)
    wrong = rng.permutation(C)[: int(0.7 * C)]
    idx[wrong] = rng.integers(0, C, len(wrong))
    return src, tgt, idx


def ransac_row(capi, ctx, src, tgt, idx, hypotheses):
    p = capi.ransac_params(0.01, hypotheses=hypotheses, seed=1)
    call, out = [], None
    for i in range(WARM + CALLS):
        t0 = time.perf_counter()
        out = ctx.ransac_register(src, tgt, idx, p)
        if i >= WARM:
            call.append((time.perf_counter() - t0) * 1e3)
    ctx.profile_enable(True)
    staged = {}
    for _ in range(STAGED):
        ctx.ransac_register(src, tgt, idx, p)
        for k, v in ctx.ransac_register_times().items():
            staged.setdefault(k, []).append(v)
    ctx.profile_enable(False)
    count_ms = median(staged["count"])
    return {"tool": "global_bench", "call": "mi_ransac_register", "hypotheses": hypotheses, "matches": len(idx), "valid_hypotheses": out[5], "inliers": out[2],
            "rmse": float(out[3]), "call_ms": round(median(call), 4), "call_ms_min": round(min(call), 4),
            "staged_ms": {k: round(median(v), 4) for k, v in staged.items()},
            "pair_tests_per_ns": round(hypotheses * float(len(idx)) / (count_ms * 1e6), 2),
            "calls": "median of %d whole calls after %d warm-up calls and of %d staged calls" % (CALLS, WARM, STAGED)}


def bumpy(n):
    """(points, unit normals): the closed surface |p| = g(p / |p|) of tests/test_gpu_global_registration.py along a Fibonacci spiral"""
    k = np.arange(n) + 0.5
    z = 1 - 2 * k / n
    phi = np.pi * (1 + 5 ** 0.5) * k
    u = np.stack([np.sqrt(1 - z * z) * np.cos(phi), np.sqrt(1 - z * z) * np.sin(phi), z], axis=1)
    ux, uy, uz = u.T
    g = 1 + 0.15 * np.sin(3 * ux + 1) + 0.1 * np.cos(4 * uy * uz + 2 * ux) + 0.08 * np.sin(5 * uz)
    s = -0.1 * np.sin(4 * uy * uz + 2 * ux)
    grad = np.stack([0.45 * np.cos(3 * ux + 1) + 2 * s, 4 * uz * s, 4 * uy * s + 0.4 * np.cos(5 * uz)], axis=1)
    nrm = u - (grad - u * (grad * u).sum(axis=1, keepdims=True)) / g[:, None]
    return u * g[:, None], nrm / np.linalg.norm(nrm, axis=1, keepdims=True)


def timed(run):
    ms, out = [], None
    for i in range(WARM + CALLS):
        t0 = time.perf_counter()
        out = run()
        if i >= WARM:
            ms.append((time.perf_counter() - t0) * 1e3)
    return round(median(ms), 4), out


def pipeline_row(capi, ctx, n):
    """the three calls of a global registration on the same clouds: a bumpy closed surface and a rotated, translated, re-ordered copy"""
    p, nr = bumpy(n)
    a = np.deg2rad(100.0)
    R0 = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    perm = np.random.default_rng(11).permutation(n)
    src, src_n = p.astype(np.float32), nr.astype(np.float32)
    tgt, tgt_n = (p @ R0.T + [0.5, -1.0, 2.0])[perm].astype(np.float32), (nr @ R0.T)[perm].astype(np.float32)
    fpfh_ms, fs = timed(lambda: ctx.fpfh_features(src, src_n, 16))
    ft = ctx.fpfh_features(tgt, tgt_n, 16)
    match_ms, idx = timed(lambda: ctx.feature_match(fs, ft, mutual=True))
    spacing = float(np.sqrt(4 * np.pi / n))
    params = capi.ransac_params(0.25 * spacing, hypotheses=100000, seed=3)
    row = {"tool": "global_bench", "call": "pipeline", "points": n, "k": 16, "mutual_matches": int((idx >= 0).sum()),
           "correct_matches": int((idx == np.argsort(perm)).sum()), "hypotheses": 100000, "max_distance": round(0.25 * spacing, 6),
           "fpfh_call_ms_one_cloud": fpfh_ms, "feature_match_call_ms": match_ms, "calls": "median of %d whole calls after %d warm-up calls" % (CALLS, WARM)}
    if row["mutual_matches"] < 3:                         # descriptors too alike at this density and k: nothing to register from
        return dict(row, ransac_register_call_ms=None)
    ransac_ms, out = timed(lambda: ctx.ransac_register(src, tgt, idx, params))
    err = np.linalg.norm(src.astype(np.float64) @ out[0].astype(np.float64).T + out[1] - (src.astype(np.float64) @ R0.T + [0.5, -1.0, 2.0]), axis=1)
    return dict(row, valid_hypotheses=out[5], inliers=out[2], worst_point_error=float(err.max()), ransac_register_call_ms=ransac_ms,
                ransac_over_fpfh=round(ransac_ms / fpfh_ms, 3))


def main():
    capi = load_package().capi
    sizes = [int(float(a)) for a in sys.argv[1:]] or [10 ** 4, 10 ** 5]
    with capi.Context(0) as ctx:
        ctx.preload()
        for rows in sizes:
            rng = np.random.default_rng(666)
            q, t = (np.ascontiguousarray(rng.uniform(0, 200, (rows, DIM)), np.float32) for _ in range(2))
            for mutual in (0, 1):
                print(json.dumps(one(capi, ctx, q, t, mutual)), flush=True)
        for C in sizes:
            src, tgt, idx = planted(np.random.default_rng(667), C)
            for hypotheses in sizes:
                print(json.dumps(ransac_row(capi, ctx, src, tgt, idx, hypotheses)), flush=True)
        for n in (3000, 10000, 30000):
            print(json.dumps(pipeline_row(capi, ctx, n)), flush=True)


if __name__ == "__main__":
    main()
