"""GPU suite: what the CPD workspace carries from one call on a context to the next -- the fixed cloud's finished sweep (swept_K), the moving
cloud's guess and its prelaunched replay, the truncated E-step's curve orders (trunc_ready), the rows of M-step partial sums an E-step left,
the read-back's last_call, the sharding flags -- must never reach a result.  One long-lived context makes the calls below in order (each picked
for a piece of that state: see the comments); every answer is compared BIT FOR BIT with the same call on a freshly created context."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REFUSAL = "mi_selftest_cpd_last: the last call on this context was no mi_cpd_register / mi_cpd_mstep"


def clouds(seed, m, n, noise=0.01):
    """A seeded cloud in a 6 x 4 x 2 box, and n points of it in another order under a known similarity transform (scale 1.05, 0.1 rad about z,
    a shift) with a little noise: a hybrid registration of the 300 x 350 pair takes about 20 iterations and its last ones the truncated E-step."""
    rng = np.random.default_rng(seed)
    base = rng.uniform(-1.0, 1.0, size=(max(m, n), 3)) * np.array([3.0, 2.0, 1.0])
    c, s = np.cos(0.1), np.sin(0.1)
    R = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    after = 1.05 * base[rng.permutation(len(base))[:n]] @ R.T + np.array([0.1, -0.05, 0.05]) + noise * rng.normal(size=(n, 3))
    return base[:m].astype(np.float32), after.astype(np.float32)


def flat(value):
    """Every number of a call's answer as bytes, in order (tuples, lists, dicts by key, arrays, scalars)."""
    if isinstance(value, dict):
        return b"".join(flat(value[k]) for k in sorted(value))
    if isinstance(value, (tuple, list)):
        return b"".join(flat(v) for v in value)
    if isinstance(value, (float, np.floating)):
        return np.float64(value).tobytes()
    if isinstance(value, (int, np.integer)):
        return np.int64(value).tobytes()
    if isinstance(value, np.ndarray):
        return np.ascontiguousarray(value).tobytes()
    return bytes(value)                                                            # a ctypes structure (the batched call's info)


def register_and_read_back(capi, ctx, before, after, **params):
    out = ctx.cpd_register(before, after, capi.cpd_params(**params))
    return out, ctx.selftest_cpd_last(len(before), len(after))


def steps(capi):
    """[(name, call)]: call(ctx) makes one step's calls on ctx and returns everything they answered."""
    # (tolerance 0: the hybrid runs go on until sigma^2 <= eps, through the switch from the FGT to the truncated E-step at 0.015 sigma^2_0)
    hybrid = dict(approximation=capi.CPD_APPROX_HYBRID, max_iterations=60, tolerance=0.0)
    b1, a1 = clouds(1, 300, 350)
    b3, a3 = clouds(3, 70, 130)
    y4, x4 = clouds(4, 400, 500, noise=0.2)
    b5, a5 = clouds(5, 200, 200)
    b5c, a5c = clouds(55, 1000, 17)
    y6, x6 = clouds(6, 65, 63)
    y6b, x6b = clouds(66, 1025, 1023)
    c8, _ = clouds(8, 300, 2)
    batch_sizes = ((64, 64), (2048, 100), (2100, 90))              # (the third: beyond the routed edge, the single path inside the batched call)
    batch = [clouds(90 + i, m, n) for i, (m, n) in enumerate(batch_sizes)]
    kept = {}

    def step1(ctx):
        return register_and_read_back(capi, ctx, b1, a1, **hybrid)

    def step4(ctx):
        kept["estep"] = ctx.cpd_estep_fgt(y4, x4, 0.3, 2.0, 4.0)
        return kept["estep"]

    def step7a(ctx):
        p1, pt1, px, _ = kept["estep"]
        return ctx.cpd_mstep(y4, x4, p1, pt1, px, False, scale=1.0, sigma2=2.0), ctx.selftest_cpd_last(400, 500)

    def step7b(ctx):
        s2 = ctx.cpd_sigma_squared(y4, x4)
        with pytest.raises(capi.MiSlamError) as refused:
            ctx.selftest_cpd_last(400, 500)
        assert REFUSAL in str(refused.value)
        return s2

    def step9(ctx, **params):
        return ctx.cpd_register_batch([b for b, _ in batch], [a for _, a in batch], capi.cpd_params(**params))

    return [
        ("1 hybrid register 300 x 350", step1),
        # the moving side's buffers now hold another cloud's sweep: the registration's guess must go
        ("2 fgt_kcenter 70, K 5", lambda ctx: ctx.fgt_kcenter(b3, 5)),
        # smaller clouds in buffers that stay: the fixed cloud's clustering starts over, no guess survives the load
        ("3 hybrid register 70 x 130", lambda ctx: register_and_read_back(capi, ctx, b3, a3, **hybrid)),
        ("4 estep_fgt 400 x 500", step4),
        # ICP shares the moving cloud's buffers (bx.., cx..) with CPD
        ("5a icp_register 200", lambda ctx: ctx.icp_register(b5, a5, capi.icp_params(max_iterations=10))),
        ("5b exact register 1000 x 17", lambda ctx: register_and_read_back(capi, ctx, b5c, a5c, max_iterations=30)),
        # the curve orders of one pair of clouds must not serve the next
        ("6a estep_truncated 65 x 63", lambda ctx: ctx.cpd_estep_truncated(y6, x6, 0.1, 0.05)),
        ("6b estep_truncated 1025 x 1023", lambda ctx: ctx.cpd_estep_truncated(y6b, x6b, 0.1, 0.05)),
        ("7a mstep 400 x 500 and its read-back", step7a),
        ("7b sigma_squared, then a read-back that is refused", step7b),
        ("8a fgt_kcenter_guided 300, K 50, 20 guessed", lambda ctx: ctx.fgt_kcenter_guided(c8, 50, np.arange(0, 300, 15, dtype=np.int32))),
        # ... and the plain call behind it replays nothing
        ("8b fgt_kcenter 300, K 50", lambda ctx: ctx.fgt_kcenter(c8, 50)),
        ("9a register_batch, exact", lambda ctx: step9(ctx, max_iterations=30)),
        ("9b register_batch, full: every problem through the single path", lambda ctx: step9(ctx, approximation=capi.CPD_APPROX_FULL, max_iterations=3)),
        ("9c hybrid register 300 x 350 again", step1),
        ("10 full register 300 x 350", lambda ctx: register_and_read_back(capi, ctx, b1, a1, approximation=capi.CPD_APPROX_FULL, max_iterations=5, tolerance=0.0)),
    ]


def test_a_reused_context_answers_as_a_fresh_one(capi):
    answers = {}
    with capi.Context(0) as reused:
        for name, call in steps(capi):
            got = call(reused)
            with capi.Context(0) as fresh:
                want = call(fresh)
            assert flat(got) == flat(want), "step %s: the reused context's answer differs from a fresh context's" % name
            answers[name] = flat(got)
            if isinstance(got, tuple) and len(got) == 2 and isinstance(got[1], dict):
                print("step %s: route %d, %d iterations, stop %d" % (name, got[1]["route"], got[1]["iterations"], got[1]["stop_reason"]))
    assert answers["9c hybrid register 300 x 350 again"] == answers["1 hybrid register 300 x 350"]
