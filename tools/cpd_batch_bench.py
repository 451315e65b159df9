#!/usr/bin/env python3
"""Times mi_cpd_register_batch against a loop of mi_cpd_register over the same seeded problems, host buffers in, results out (the
whole_call convention of tools/whole_call.py), and prints one JSON line per (B, size) with the medians and spreads of both.

    python tools/cpd_batch_bench.py --sizes 256,512,1024,2048,4096 --batches 1,16,64,256,1024 [--baseline-lib path/to/parent/libmislam.so]

The loop of single calls runs on --baseline-lib when given (the parent commit's build, next to this one: tools/gpu_ab.sh shows how two
builds are kept side by side), else on this build.  The two are alternated --reps times (>= 5); every timed window lasts at least
--min-seconds."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,512,1024,2048,4096")
    ap.add_argument("--batches", default="1,16,64,256,1024")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--max-iterations", type=int, default=30)
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    import __graft_entry__
    capi = __graft_entry__.load_package().capi
    import icp_batch_catalogue as cat

    base = C.CDLL(args.baseline_lib) if args.baseline_lib else capi.lib()
    base.mi_cpd_register.restype = C.c_int
    h = C.c_void_p()
    assert base.mi_ctx_create(0, C.byref(h)) == 0
    ctx = capi.Context(0)
    params = capi.cpd_params(max_iterations=args.max_iterations)
    fp = C.POINTER(C.c_float)

    def loop(problems):
        T = (C.c_float * 16)()
        it, err, sc = C.c_int(0), C.c_float(0), C.c_float(0)
        for b, a in problems:
            rc = base.mi_cpd_register(h, b.ctypes.data_as(fp), len(b), a.ctypes.data_as(fp), len(a), C.byref(params), T, C.byref(sc), C.byref(it), C.byref(err))
            assert rc == 0

    def window(fn):
        fn()                                            # warm
        n, t0 = 0, time.perf_counter()
        while True:
            fn()
            n += 1
            dt = time.perf_counter() - t0
            if dt >= args.min_seconds:
                return 1e3 * dt / n

    for size in [int(s) for s in args.sizes.split(",")]:
        pool = [cat.pair(args.seed + k, size, size) for k in range(16)]
        for B in [int(b) for b in args.batches.split(",")]:
            problems = [pool[k % len(pool)] for k in range(B)]
            before = np.concatenate([b for b, _ in problems])
            after = np.concatenate([a for _, a in problems])
            r = np.stack([np.arange(B) * size, np.full(B, size)], 1)
            info = []
            batched_fn = lambda: info.append(ctx.cpd_register_batch(before, after, params, before_range=r, after_range=r)[6])
            tb, ts = [], []
            for _ in range(max(args.reps, 1)):
                ts.append(window(lambda: loop(problems)))
                tb.append(window(batched_fn))
            med_s, med_b = float(np.median(ts)), float(np.median(tb))
            print(json.dumps({"tool": "cpd_batch_bench", "B": B, "m": size, "n": size, "max_iterations": args.max_iterations,
                              "baseline": "parent" if args.baseline_lib else "this build",
                              "loop_ms": round(med_s, 4), "loop_spread_ms": round(max(ts) - min(ts), 4),
                              "batched_ms": round(med_b, 4), "batched_spread_ms": round(max(tb) - min(tb), 4),
                              "ratio_loop_over_batched": round(med_s / med_b, 3), "launches": info[-1].launches,
                              "problems_batched": info[-1].problems_batched, "reps": args.reps}), flush=True)
    base.mi_ctx_destroy(h)
    ctx.close()


if __name__ == "__main__":
    main()
