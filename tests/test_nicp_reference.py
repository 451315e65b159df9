"""CPU suite: pins tests/nicp_reference.py -- the float64 restatement tests/test_gpu_nicp_stages.py holds the device to -- against the plain-C
restatement of the reference (oracle/nicp_oracle.c), so that the GPU suite's reference cannot be wrong unnoticed.

Measured here (printed with -s): the oracle's own max ||U_a^T R U_b| - I| is 2e-7 .. 1.1e-6 on clouds of 4 .. 4000 points (fp32 QR and Jacobi
sweeps over N points), against 16 * 2^-23 / gap = 5e-6 .. 3e-5 allowed."""
import numpy as np
import pytest

import nicp_reference as N
from test_nicp_oracle import rigid_pair


def oracle_candidate(oracle, b, a, head):
    pb, pa = N.permuted(b, a, N.full_permutation(head, min(len(b), len(a))))
    return oracle.nicp_single(pb, pa)


def loose(seed, n):                                                  # the non-rigid pairs of test_nicp_oracle.test_single_matches_reference
    rng = np.random.default_rng(seed)
    b = (rng.normal(size=(n, 3)) * rng.uniform(0.5, 3, 3)).astype(np.float32)
    a = (rng.normal(size=(n, 3)) * rng.uniform(0.5, 3, 3) + rng.normal(size=3)).astype(np.float32)
    return b, a


CLOUDS = [("rigid", 1, 2500, 0.01), ("rigid", 3, 64, 0.05), ("rigid", 5, 3000, 0.0), ("rigid", 6, 1800, 0.01)] + \
         [("loose", s, n, None) for s, n in ((0, 5), (1, 7), (2, 50), (3, 1000), (4, 4000))]


@pytest.mark.parametrize("kind,seed,n,noise", CLOUDS)
def test_axes_and_approximated_error_against_the_oracle(oracle, kind, seed, n, noise):
    b, a = rigid_pair(seed, n, noise)[:2] if kind == "rigid" else loose(seed, n)
    c = N.centred(b, a)
    (Ub, _, gb), (Ua, _, ga) = N.axes(c["Gb"]), N.axes(c["Ga"])
    gap = min(gb.min(), ga.min())
    rng = np.random.default_rng(seed)
    for head in [np.arange(3)] + [rng.permutation(n)[:3] for _ in range(3)]:
        R, t, e = oracle_candidate(oracle, b, a, head)
        D = Ua.T @ R.astype(np.float64) @ Ub
        dev = np.abs(np.abs(D) - np.eye(3)).max()
        ref = N.approx_error(R, b, a)
        print("%s n=%d gap %.3f: | |D| - I | %.2e (allowed %.2e), approx %.6e against %.6e" % (kind, n, gap, dev, 16 * N.EPS32 / gap, e, ref))
        assert dev <= 16 * N.EPS32 / gap                              # diagonal, entries of magnitude 1
        # 5e-6: test_single_matches_reference's tolerance; where the residual is the rounding of the inputs alone (a noise-free rigid pair's
        # right candidate) the oracle's fp32 chain has nothing to agree on: the centred points' own rounding, 2^-23 of their size, squared
        assert abs(e - ref) <= 5e-6 * ref + (4 * N.EPS32 * np.abs(a).max()) ** 2
        assert abs(N.approx_from_sums(R, c) - ref) <= N.EPS32 * ref + N.approx_floor(c)     # the expansion on centred sums: the floor holds


def oracle_numbers(oracle, b, a, heads, sub):
    """The oracle's own candidates and their two errors, one repetition at a time."""
    size = min(len(b), len(a))
    perms = np.stack([N.full_permutation(h, size) for h in heads])
    cands, approx, exact = [], [], []
    for k in range(len(heads)):
        R, t, e = oracle_candidate(oracle, b, a, heads[k])
        _, _, _, err = oracle.nicp(b, a, perms[k:k + 1], sub, -1.0, 1, 0)
        cands.append(R.tobytes() + t.tobytes())
        approx.append(np.float32(e))
        exact.append(np.float32(err))
    return perms, cands, approx, exact


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("eps", [1e-9, 1e-3])
@pytest.mark.parametrize("order", ["falling", "mixed"])
@pytest.mark.parametrize("m,n", [(257, 257), (1000, 2500)])
def test_driver_reproduces_the_oracles_pick(oracle, m, n, order, eps, mode):
    b, a, heads, sub = N.pick_case(m, n, order)
    perms, cands, approx, exact = oracle_numbers(oracle, b, a, heads, sub)
    assert len(set(cands)) == 8 and len(set(np.array(approx).tolist())) >= 7       # one tie, a list that can overflow
    d = N.driver(list(range(9)), approx, exact, eps, mode)
    Ro, to, no, eo = oracle.nicp(b, a, perms, sub, eps, 9, mode)
    assert d["repetitions"] == no
    assert cands[d["winner"]] == Ro.tobytes() + to.tobytes()
    assert np.float32(d["error"]) == np.float32(eo)
    if mode == 2 and order == "falling":
        assert d["overflowed"] and len(d["listed"]) == 5
    if mode == 0 and order == "mixed" and eps == 1e-3 and m == n:
        assert d["repetitions"] == 5                                               # the early exit, at the best candidate's repetition


@pytest.mark.parametrize("order", ["falling", "mixed"])
@pytest.mark.parametrize("m,n", [(257, 257), (1000, 2500)])
def test_pick_cases_have_no_near_ties_of_the_exact_error(oracle, m, n, order):
    # what lets tests/test_gpu_nicp_stages.py demand the same winner of every case: no two different candidates score within 2^-22 of each
    # other on the restatement, and no score lies that close to a threshold in use
    b, a, heads, sub = N.pick_case(m, n, order)
    cands = [oracle_candidate(oracle, b, a, h) for h in heads]
    errors = [N.exact_error(R, t, b[sub], a)[0] for R, t, _ in cands]
    assert N.near_ties(errors, [R.tobytes() + t.tobytes() for R, t, _ in cands]) == []
    for eps in (1e-9, 1e-3):
        assert all(abs(e - eps) > 2.0 ** -20 * eps for e in errors)


def test_store_if_optimal_quirks():
    lst = []
    for k, e in enumerate([5.0, 4.0, 4.0, 3.0]):
        N.store_if_optimal(lst, k, np.float32(e), 5)
    # 4 beats 5: [1, 0]; the second 4 beats only 5: [1, 2, 0]; 3 beats the entry at 0, is inserted there, meets the same entry again at 1 and
    # at 2 and is inserted before it each time, until the sixth entry overflows the list and its tail is cut
    assert [k for k, _ in lst] == [3, 3, 3, 1, 2]
    one = []
    for k, e in enumerate([5.0, 5.0, 4.0]):
        N.store_if_optimal(one, k, np.float32(e), 1)
    assert [k for k, _ in one] == [2]
    d = N.driver([0, 1, 2], [1.0, 1.0, 1.0], [np.nan, np.nan, np.nan], 1e-3, 0)
    assert d["winner"] == 0 and d["error"] == N.FLT_MAX and d["repetitions"] == 3  # nothing within the limit: the first candidate scored


def test_exact_error_is_the_oracles_subcloud_score(oracle):
    b, a, heads, sub = N.pick_case(257, 257, "mixed")
    perms = np.stack([N.full_permutation(h, 257) for h in heads])
    for k in (0, 4):
        R, t, _ = oracle_candidate(oracle, b, a, heads[k])
        mean, kept, idx, d2 = N.exact_error(R, t, b[sub], a)
        err = oracle.nicp(b, a, perms[k:k + 1], sub, -1.0, 1, 0)[3]
        assert kept == len(sub) and abs(mean - err) <= len(sub) * N.EPS32 * mean   # the oracle sums its d2 sequentially in fp32
    far = (b[:4] * 1e-3 + 5000.0).astype(np.float32)
    assert N.exact_error(np.eye(3, dtype=np.float32), np.zeros(3, np.float32), far, a)[:2][1] == 0


# ---- how far from the origin: the host's formula in float64 on sums about the first points, and on raw coordinates ----
OFFSETS = (1e2, 1e3, 1e4, 1e5)


def _within_bounds(b, a, about_first):
    """(worst |approx - reference| / bound d, worst axes deviation / bound b) of the formula alone, over the eight sign patterns."""
    c = N.centred(b, a)
    s, _ = N.moments(b, a, about_first=about_first)
    r = N.sums_from_raw(np.asarray(s, np.float64), len(b), len(a))
    (Ub, _, gb), (Ua, _, ga) = N.axes(c["Gb"]), N.axes(c["Ga"])
    worst_d = 0.0
    for signs in np.ndindex(2, 2, 2):                               # all eight: the one that fits the rigid pair is among them
        signs = 1 - 2 * np.array(signs)
        R = ((Ua * signs) @ Ub.T).astype(np.float32)
        ref = N.approx_error(R, b, a)
        worst_d = max(worst_d, abs(N.approx_from_sums(R, r) - ref) / (N.EPS32 * ref + N.approx_floor(c)))
    dev = max(np.abs(np.abs(U.T @ N.axes(G)[0]) - np.eye(3)).max() for U, G in ((Ub, r["Gb"]), (Ua, r["Ga"])))
    rel = max(np.abs(r[k] - c[k]).max() / np.abs(c[k]).max() for k in ("Gb", "Ga"))
    return worst_d, dev / (16 * N.EPS32 / min(gb.min(), ga.min())), rel


@pytest.mark.parametrize("noise", [0.0, 0.01])
def test_sums_about_the_first_point_hold_the_bounds_at_every_offset(noise):
    for offset in OFFSETS:
        b, a = N.rigid_pair(17507, 2500, 2500, noise, np.full(3, offset))
        d, ax, rel = _within_bounds(b, a, True)
        d0, ax0, rel0 = _within_bounds(b, a, False)
        print("offset %g noise %g: about the first point d %.2e axes %.2e Gram %.2e | raw coordinates d %.2e axes %.2e Gram %.2e" % (offset, noise, d, ax, rel, d0, ax0, rel0))
        assert d <= 1.0 and ax <= 1.0 and rel <= 1e-13
        if offset >= 1e3:
            assert d0 > 1.0                                         # why the kernel takes an origin: raw coordinates miss bound d from 1e3 on
    for m in (4, 5, 63):                                            # ... and small noise-free clouds miss it at (100, -50, 25) already
        b, a = N.rigid_pair(m * 8, m, m, 0.0, N.SHIFT)
        assert _within_bounds(b, a, True)[0] <= 1.0 < _within_bounds(b, a, False)[0]
