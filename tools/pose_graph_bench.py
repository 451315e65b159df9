"""mi_pose_graph_optimize on synthetic maps of V = 1e4 and 1e5 poses, E = (V - 1) + 4 V edges (an odometry chain and four random loop
closures per node), measurements made from the truth, the start disturbed by 0.02 rad and 0.1 units per node.

Prints, per size: the whole call (median, min - max of the repeats after the warm-ups, profiling off), the stages of mi_pose_graph_times
(median of the profiled repeats: the stream is drained after every stage), the report, one linearisation (edge kernel + node gather + the
cost's read-back: mi_pose_graph_system's stage 3) and the inner solve per conjugate-gradient iteration (the product kernel, the two vector
kernels and the two scalar kernels: stage 4 of a mi_pose_graph_system call with solve, over its iteration count).  The product kernel's
algorithmic traffic per iteration -- per list entry 21 doubles of M, two p rows of 6 and the entry's int, per node the 6 doubles of q and
of the block's diagonal -- divided by that per-iteration time is a LOWER bound of what the kernel alone moves per second; it stands
beside the 8 TB/s HBM peak of an MI355X.  The kernels are not timed one by one: that takes rocprofv3 --kernel-trace around this script.

    python tools/pose_graph_bench.py [--sizes 10000 100000] [--repeats 5] [--warmup 1]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import pose_graph_reference as P          # noqa: E402  (the graphs' generators)
from __graft_entry__ import load_package  # noqa: E402

HBM_PEAK = 8.0e12


def T44(R, t):
    T = np.zeros((len(R), 4, 4))
    T[:, :3, :3], T[:, :3, 3], T[:, 3, 3] = R, t, 1.0
    return T


def graph(V, seed=1):
    rng = np.random.default_rng(seed)
    src, tgt = P.random_graph_edges(rng, V, 4 * V)
    R, t = P.random_poses(rng, V)
    Rz, tz = P.measure(R, t, src, tgt)
    d = np.concatenate([0.02 * rng.normal(size=(V, 3)), 0.1 * rng.normal(size=(V, 3))], axis=1)
    d[0] = 0.0
    R0, t0 = P.update(R, t, d)
    return dict(truth=T44(R, t), start=T44(R0, t0), src=src, tgt=tgt, Z=T44(Rz, tz), info=P.random_information(rng, len(src)))


def spread(xs):
    return "%.3f (%.3f - %.3f)" % (float(np.median(xs)), min(xs), max(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[10000, 100000])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    capi = load_package().capi
    with capi.Context(0) as ctx:
        for V in a.sizes:
            g = graph(V)
            E = len(g["src"])
            args = (g["start"], g["src"], g["tgt"], g["Z"], g["info"])
            F0 = ctx.pose_graph_system(*args)["cost"]
            params = capi.pose_graph_params(absolute_cost=1e-18 * F0, max_pcg_iterations=2000)
            whole, stages = [], []
            for i in range(a.warmup + a.repeats):
                t0 = time.perf_counter()
                poses, w, chi2, rep = ctx.pose_graph_optimize(*args, params=params)
                if i >= a.warmup:
                    whole.append(1e3 * (time.perf_counter() - t0))
            ctx.profile_enable(True)
            for i in range(a.repeats):
                ctx.pose_graph_optimize(*args, params=params)
                stages.append(ctx.pose_graph_times())
            per_iteration, linearise = [], []
            for i in range(a.repeats):
                o = ctx.pose_graph_system(*args, params=params, solve=True)
                ms = ctx.pose_graph_times()
                linearise.append(ms["linearise"])
                per_iteration.append(ms["solve"] / max(1, o["pcg_iterations"]))
            ctx.profile_enable(False)
            err = float(np.abs(poses - g["truth"]).max())
            bytes_per_iteration = 2 * E * (8 * (21 + 12) + 4) + V * 8 * 12
            it_ms = float(np.median(per_iteration))
            print("V = %d, E = %d: whole call %s ms; report %s; worst pose entry against the truth %.3g" % (V, E, spread(whole), rep, err))
            print("  stages, ms: " + ", ".join("%s %.3f" % (k, float(np.median([s[k] for s in stages]))) for k in stages[0]))
            print("  one linearisation %s ms; inner solve %s ms per iteration over %d iterations" % (spread(linearise), spread(per_iteration), o["pcg_iterations"]))
            print("  product kernel: %.1f algorithmic bytes per edge and iteration, %.2f MB per iteration; over the whole iteration's time %.1f GB/s "
                  "(a lower bound for the kernel alone), %.2f %% of the %.0f TB/s HBM peak" % (bytes_per_iteration / E, bytes_per_iteration / 1e6,
                                                                                             bytes_per_iteration / (it_ms * 1e-3) / 1e9,
                                                                                             100 * bytes_per_iteration / (it_ms * 1e-3) / HBM_PEAK, HBM_PEAK / 1e12))


if __name__ == "__main__":
    main()
