"""bench.py's plain run and --dump-outputs: a plain run reports the timed steps only, and what it dumps is the registration the timed
steps computed -- the same R, t, error and iteration count a caller of the library gets from the same inputs and the same calls."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, synth_cloud

FULL_ONLY = ("ms_per_step_without_events", "library_default_batch", "kernels_ms_per_step", "late_iterations", "sizes", "bruteforce_nn",
             "cpd_bunny", "whole_call", "cpu_baseline", "allreduce_f64_sum_floor", "target_sharded")


def bench(args, timeout):
    env = dict(os.environ, OMP_NUM_THREADS="1")
    for v in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(v, None)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, cwd=ROOT, capture_output=True, text=True,
                          timeout=timeout)


@pytest.mark.parametrize("args", [["--steps", "0"], ["--warmup", "-1"]])
def test_bench_rejects_a_run_without_timed_steps(args):
    r = bench(args, 120)
    assert r.returncode != 0 and "{" not in r.stdout


@pytest.mark.gpu
def test_plain_bench_dumps_what_its_timed_steps_computed(ctx, capi, tmp_path):
    steps, warmup, n = 4, 2, 60000
    r = bench(["--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--points", str(n), "--dump-outputs", str(tmp_path)], 600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-4000:]
    out = json.loads(lines[0])
    assert out["metric"] == "icp_iterations_per_s" and out["unit"] == "iterations/s" and out["higher_is_better"] is True and out["dtype"] == "f32"
    assert out["steps"] == steps and out["warmup"] == warmup and out["value"] > 0
    assert abs(out["ms_per_step"] - 1e3 / out["value"]) <= 1e-9 * out["ms_per_step"]
    assert not [k for k in FULL_ONLY if k in out], out.keys()
    got = {name: np.load(str(tmp_path / (name + ".npy"))) for name in ("icp_R", "icp_t", "icp_error", "icp_iterations")}
    assert got["icp_R"].dtype == np.float32 and got["icp_R"].shape == (3, 3)
    assert got["icp_t"].dtype == np.float32 and got["icp_t"].shape == (3,)
    assert got["icp_error"].dtype == np.float32 and got["icp_iterations"].dtype == np.float64
    # the same inputs (the bench's seeded recipe) through the same calls: warm-up, then the timed steps with one host check behind them
    before, after, _, _ = synth_cloud(n)
    ctx.icp_load(before, after, capi.icp_params(eps=0.0, max_iterations=-1, dist_mode=capi.DIST_CPU_ROUNDING, nn_mode=capi.NN_AUTO,
                                                shard_mode=capi.SHARD_AUTO, sync_every=steps))
    ctx.icp_run(warmup)
    assert ctx.icp_run(steps) == steps
    R, t, it, err, _ = ctx.icp_result()
    assert it == warmup + steps and got["icp_iterations"][0] == it
    assert np.array_equal(got["icp_R"], R) and np.array_equal(got["icp_t"], t) and got["icp_error"][0] == np.float32(err)
    assert out["config"]["error_after_steps"] == err
