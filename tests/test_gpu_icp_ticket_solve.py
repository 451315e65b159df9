"""GPU suite: above the one-workgroup size the rows reduction's LAST summing workgroup runs the deferred solve (icp_rows_reduce_solve_kernel: an
arrival ticket, nobody waits) instead of a second launch.  MISLAM_ICP_TICKET_SOLVE=0, read at context creation, keeps the two launches: the two
forms must agree bit for bit -- the solving wave reads the same reduced rows back from memory and adds them in the same butterfly -- the ticket
must be back at zero behind every launch, and the work order dealt beside the sums must stay a permutation (its cursors now come in two pairs,
one per step parity, because the solving wave can no longer zero the pair the launch's own dealing workgroups are still using).

The stop-rule case takes its eps from the two-launch form's own error trajectory (between the errors of iterations 3 and 4), so that the rule
fires at iteration 4 by construction; every comparison is `==` on the bytes.
"""
import os
import re

import numpy as np
import pytest

from conftest import ROOT, synth_cloud

pytestmark = pytest.mark.gpu


def _kernels_h(name):
    text = open(os.path.join(ROOT, "cuda-slam_amd", "csrc", "kernels.h")).read()
    return int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))


MAX_ROWS = _kernels_h("ICP_FUSED_SOLVE_MAX_ROWS")      # up to here one workgroup does both (icp_reduce_solve_kernel)
REDUCED = _kernels_h("ICP_REDUCED_ROWS")               # summing workgroups at most
CHUNK = _kernels_h("ICP_CHUNK_POINTS")                 # moving points per row


def rows_of(n):
    return (n + CHUNK - 1) // CHUNK


def reduced_count(nrows):                              # icp_reduced_count (icp_kernels.hip): ~32 rows per workgroup, at most REDUCED
    return max(1, min(REDUCED, (nrows + 31) // 32))


N_THRESHOLD = CHUNK * MAX_ROWS + CHUNK                 # the smallest cloud that takes the new kernel: one row past the one-workgroup form
N_RAGGED = CHUNK * (MAX_ROWS + 140) - 17               # rows no multiple of the summing workgroups: a short last slice, and a partly filled last row
SIZES = [N_THRESHOLD, N_RAGGED, 262144, 300001]


def test_sizes_exercise_what_they_are_named_for():
    assert rows_of(N_THRESHOLD) == MAX_ROWS + 1
    r = rows_of(N_RAGGED)
    assert r > MAX_ROWS and r % reduced_count(r) != 0 and N_RAGGED % CHUNK != 0
    assert rows_of(262144) == 4096 and reduced_count(4096) == REDUCED and 4096 // REDUCED == 64       # more than one row per strip (56 strips)
    assert rows_of(300001) == 4688 and reduced_count(4688) == REDUCED and 300001 % CHUNK != 0                  # (an odd tail: a partly filled last row)


@pytest.fixture(scope="module")
def forms(capi):
    """(ticket form, two-launch form): two contexts that differ in MISLAM_ICP_TICKET_SOLVE alone."""
    saved = os.environ.get("MISLAM_ICP_TICKET_SOLVE")
    try:
        os.environ["MISLAM_ICP_TICKET_SOLVE"] = "1"
        one = capi.Context(0)
        os.environ["MISLAM_ICP_TICKET_SOLVE"] = "0"
        two = capi.Context(0)
    finally:
        if saved is None:
            os.environ.pop("MISLAM_ICP_TICKET_SOLVE", None)
        else:
            os.environ["MISLAM_ICP_TICKET_SOLVE"] = saved
    yield one, two
    one.close()
    two.close()


_clouds = {}


def clouds(n):
    if n not in _clouds:
        _clouds[n] = synth_cloud(n, seed=n)[:2]
    return _clouds[n]


def snapshot(c):
    """Everything a registration leaves: R, t, iterations, error, stop reason and the raw sums of the last solve, as bytes."""
    R, t, it, err, why = c.icp_result()
    s = c.selftest_icp_schedule()
    return (R.tobytes(), t.tobytes(), it, np.float32(err).tobytes(), why, s["sums"].tobytes()), s


def register(c, before, after, p, budget=-1):
    c.icp_load(before, after, p)
    c.icp_run(budget)
    return snapshot(c)


@pytest.mark.parametrize("n", SIZES)
def test_ticket_form_is_the_two_launch_form_bit_for_bit(forms, capi, n):
    one, two = forms
    before, after = clouds(n)
    want = None
    for sync in (1, 5, 12):
        p = capi.icp_params(eps=0.0, max_iterations=12, sync_every=sync)
        a, sa = register(one, before, after, p)
        b, _ = register(two, before, after, p)
        assert a[2] == b[2] == 12, (n, sync)
        assert a == b, (n, sync)
        assert sa["ticket"] == 0, (n, sync)
        want = want or b
        assert b == want, (n, sync)                  # (and neither form depends on the host's check interval)


def test_stop_rule_fires_alike_and_later_runs_are_no_ops(forms, capi):
    one, two = forms
    n = N_RAGGED
    before, after = clouds(n)
    # the two-launch form's error after each iteration, one host check per iteration
    two.icp_load(before, after, capi.icp_params(eps=0.0, max_iterations=-1, sync_every=1))
    errs = []
    for _ in range(6):
        assert two.icp_run(1) == 1
        errs.append(two.icp_result()[3])
    assert all(errs[i] > errs[i + 1] for i in range(4)), errs
    eps = float(np.float32(0.5 * (errs[3] + errs[4])))          # above iteration 4's error (index 4), below every earlier one
    assert errs[4] < eps < errs[3]
    for sync in (1, 5, 12):                                       # 12: the rule fires in the middle of a batch
        p = capi.icp_params(eps=eps, max_iterations=-1, sync_every=sync)
        a, sa = register(one, before, after, p, budget=12)
        b, _ = register(two, before, after, p, budget=12)
        assert a == b, sync
        assert a[4] == capi.STOP_CONVERGED and np.frombuffer(a[3], np.float32)[0] == np.float32(errs[4]), (sync, a[2])
        assert sa["ticket"] == 0
        for c, first in ((one, a), (two, b)):
            assert c.icp_run(5) == 0
            again, s = snapshot(c)
            assert again == first and s["ticket"] == 0


def test_ticket_returns_to_zero_and_a_context_can_be_used_again(forms, capi):
    one, _ = forms
    n = N_THRESHOLD
    before, after = clouds(n)
    p = capi.icp_params(eps=0.0, max_iterations=7, sync_every=3)
    with capi.Context(0) as fresh:
        want, s = register(fresh, before, after, p)
        assert s["ticket"] == 0
    for _ in range(2):                                            # back to back on one context: the second as a fresh context's
        got, s = register(one, before, after, p)
        assert got == want and s["ticket"] == 0
    # ... also behind a registration whose stop rule fired in the middle of a batch
    one.icp_load(before, after, capi.icp_params(eps=0.0, max_iterations=-1, sync_every=1))
    one.icp_run(3)
    eps = float(np.nextafter(np.float32(one.icp_result()[3]), np.float32(np.inf)))       # fires at the third iteration
    stopped, s = register(one, before, after, capi.icp_params(eps=eps, max_iterations=-1, sync_every=8), budget=8)
    assert stopped[4] == capi.STOP_CONVERGED and s["ticket"] == 0
    got, s = register(one, before, after, p)
    assert got == want and s["ticket"] == 0


def test_dealt_work_order_stays_a_permutation(forms, capi):
    one, two = forms
    n = 262144
    before, after = clouds(n)
    nrows = rows_of(n)
    p = capi.icp_params(eps=0.0, max_iterations=-1, sync_every=1)
    one.icp_load(before, after, p)
    two.icp_load(before, after, p)
    for step in range(3):
        assert one.icp_run(1) == 1 and two.icp_run(1) == 1
        s, s2 = one.selftest_icp_schedule(), two.selftest_icp_schedule()
        far = s["far"] != 0
        n_far = int(far.sum())
        print("step %d: %d of %d chunks walked" % (step, n_far, nrows))
        assert len(s["order"]) == nrows and np.array_equal(np.sort(s["order"]), np.arange(nrows)), step
        assert far[s["order"][:n_far]].all() and not far[s["order"][n_far:]].any(), step          # walking chunks first, the others behind
        pair = 2 * (step & 1)                                      # the cursors this step dealt on: how many of each class it placed
        assert s["cursors"][pair] == n_far and s["cursors"][pair + 1] == nrows - n_far, (step, s["cursors"])
        assert not s["cursors"][2 - pair:4 - pair].any(), (step, s["cursors"])                     # the other pair: zeroed for the next step
        assert s["ticket"] == 0
        # the two-launch form: same flags, a permutation with the same split, every cursor zeroed by its solve launch
        assert np.array_equal(s2["far"], s["far"]) and np.array_equal(np.sort(s2["order"]), np.arange(nrows))
        assert (s2["far"][s2["order"][:n_far]] != 0).all() and not s2["cursors"].any()
