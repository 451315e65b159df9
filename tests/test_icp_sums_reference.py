"""CPU: tests/icp_sums_reference.py against the oracle on the bunny's first iteration, and the mutation checks that show what the bounds of
tests/test_gpu_icp_sums.py can see: at every size and reducer route that suite uses, a sum with one pair dropped, one pair's a_r b_c
transposed, one coordinate off by one fp32 ulp or one dropped pair counted leaves its bound in at least one of the 18 columns -- for EVERY
pair of the cloud, not a sample."""
import numpy as np
import pytest

import icp_sums_reference as S


def test_moments_and_solve_reproduce_the_oracle_on_the_bunny(oracle, golden, bunny):
    before, after = bunny
    g = golden.npz("bunny_icp_iter0.npz")
    ib, ia = g["idx_before"], g["idx_after"]
    use = np.zeros(len(before), bool)
    use[ib] = True
    matched = np.zeros_like(before)
    matched[ib] = after[ia]
    mom, mag = S.moments(before, matched, use)
    assert mom[0] == len(ib) and (mag >= np.abs(mom)).all()
    sol = S.solve(mom)
    assert sol["well"]
    Ro, to = oracle.least_squares_svd(before[ib], after[ia])
    # the bars of test_kabsch_matches_oracle_and_golden (tests/test_gpu_icp.py): the oracle's and the reference's own first solve
    assert np.abs(sol["R"] - Ro).max() < 5e-6 and np.abs(sol["t"] - to).max() < 5e-6
    assert np.abs(sol["R"] - g["R0"]).max() < 5e-6 and np.abs(sol["t"] - g["t0"]).max() < 5e-6
    # from the identity both composition rules give the solve itself
    for mode in (0, 1):
        R, t = S.compose(np.eye(3), np.zeros(3), sol["R"], sol["t"], mode)
        assert np.array_equal(R, sol["R"]) and np.array_equal(t, sol["t"])


def test_error_sums_reproduce_the_oracle_on_the_bunny(oracle, golden, bunny):
    before, after = bunny
    g = golden.npz("bunny_icp_iter0.npz")
    ib, ia = g["idx_before"], g["idx_after"]
    new = S.transform(before, g["R0"], g["t0"])
    assert np.array_equal(new, oracle.transform_cloud(before, g["R0"], g["t0"]))          # the same operations in the same order
    kept = np.zeros(len(before), bool)
    kept[ib] = True
    matched = np.zeros_like(before)
    matched[ib] = after[ia]
    err, mag = S.error_sums(matched, new, kept)
    assert err[1] == len(ib) and mag[0] == err[0]
    ref = oracle.mse_indexed(new, after, ib, ia)
    # test_transform_bit_exact_and_mse's bar: extended precision here, one sequential fp32 sum there
    assert abs(float(err[0] / err[1]) - ref) < 2e-6 * ref


def test_composition_rules():
    R, Ri = S.rotation(0.3), S.rotation(-0.1)
    t, ti = np.array([1.0, -2.0, 0.5]), np.array([0.25, 0.5, -1.0])
    x = np.array([0.3, 0.7, -1.1])
    R1, t1 = S.compose(R, t, Ri, ti, 1)
    assert np.allclose(R1 @ x + t1, Ri @ (R @ x + t) + ti, rtol=0, atol=1e-15)             # exact: T <- Ti T
    R0, t0 = S.compose(R, t, Ri, ti, 0)
    assert np.array_equal(R0, R1) and np.array_equal(t0, ti + t)                           # cpu-slam's additive translation


def test_the_counted_chains():
    # one workgroup: 18 in the row, 33 over a slice, 6 in the butterfly; the ticket and two-launch forms: a strip of ceil(slice / 56) rows, 55 strips
    assert S.additions(1, "one_workgroup") == 18 + 33 + 6 == S.additions(64 * 2048, "one_workgroup")
    assert S.additions(S.N_THRESHOLD, "ticket") == 18 + 1 + 55 + 6 == S.additions(S.N_RAGGED, "two_launch")
    assert S.additions(64 * 64 * 57, "two_launch") == 18 + 2 + 55 + 6                                       # 57 rows per slice: two in the first strip
    assert S.additions(4097, "world1", world=4) == S.additions(4097, "two_launch") + 3
    with pytest.raises(AssertionError):
        S.additions(S.N_THRESHOLD, "one_workgroup")
    assert "one_workgroup" not in S.routes_at(S.N_THRESHOLD) and "one_workgroup" in S.routes_at(64 * 2048)


def test_all_zero_terms_and_counts_have_no_tolerance():
    mag = np.zeros(16)
    assert (S.bounds(4097, "two_launch", mag) == 0).all()
    mag[:] = 1.0
    assert S.bounds(4097, "two_launch", mag)[0] == 0 and (S.bounds(4097, "two_launch", mag)[1:] > 0).all()
    assert S.bounds(4097, "two_launch", np.ones(2))[1] == 0


_cases = {}


def case(n):
    """The first iteration of the GPU suite's registration of n moving points, on the CPU: pairs, filter, exact sums."""
    if n not in _cases:
        before, after = S.clouds(n)
        idx, d2 = S.nearest(before, after)
        use = d2 < np.float32(S.median_filter(d2))
        matched = after[idx]
        mom, mom_mag = S.moments(before, matched, use)
        new = S.transform(before, S.rotation(0.02), np.array([0.01, -0.02, 0.015]))       # some small update, as a solve would apply
        err, err_mag = S.error_sums(matched, new, use)
        _cases[n] = dict(before=before, matched=matched, use=use, new=new, mom_mag=mom_mag, err_mag=err_mag)
    return _cases[n]


def route_bounds(n, route, c):
    return S.bounds(n, route, c["mom_mag"]), S.bounds(n, route, c["err_mag"])


PAIRS = [(n, route) for n in S.SIZES for route in S.routes_at(n)]


@pytest.mark.parametrize("n,route", PAIRS)
def test_dropping_any_pair_is_seen(n, route):
    c = case(n)
    bm, be = route_bounds(n, route, c)
    T = S.pair_terms(c["before"], c["matched"])[c["use"]]
    assert (np.abs(T[:, 0]) > bm[0]).all()                                  # the count alone
    assert (np.abs(T[:, 1:]) > bm[1:]).any(axis=1).all()                    # and, were the count right, the coordinates
    e = S.pair_errors(c["matched"], c["new"])[c["use"]].astype(np.float64)
    assert (e > be[0]).all() and be[1] == 0                                 # the error sum, and its count


@pytest.mark.parametrize("n,route", PAIRS)
def test_transposing_any_pairs_products_is_seen(n, route):
    c = case(n)
    bm, _ = route_bounds(n, route, c)
    T = S.pair_terms(c["before"], c["matched"])[c["use"]][:, 7:].reshape(-1, 3, 3)
    delta = np.abs(T - T.transpose(0, 2, 1)).reshape(-1, 9)                 # a_c b_r in the place of a_r b_c
    assert (delta > bm[7:]).any(axis=1).all()


@pytest.mark.parametrize("n,route", PAIRS)
def test_one_ulp_of_any_coordinate_is_seen(n, route):
    c = case(n)
    bm, _ = route_bounds(n, route, c)
    use = c["use"]
    # the smaller of a float32's two neighbouring gaps; it lands unchanged in the coordinate's own sum
    for points, cols in ((c["before"], slice(1, 4)), (c["matched"], slice(4, 7))):
        ulp = 0.5 * np.spacing(np.abs(points[use])).astype(np.float64)
        assert (ulp > bm[cols]).all(), (n, route, float(ulp.min()), bm[cols])


@pytest.mark.parametrize("n,route", PAIRS)
def test_counting_a_dropped_pair_is_seen(n, route):
    c = case(n)
    dropped = ~c["use"]
    assert dropped.any() == (n > 1)
    bm, be = route_bounds(n, route, c)
    T = S.pair_terms(c["before"], c["matched"])[dropped]
    assert (np.abs(T[:, 0]) > bm[0]).all() and (np.abs(T[:, 1:]) > bm[1:]).any(axis=1).all()
    assert be[1] == 0                                                       # one more kept pair: the error count has no tolerance either


def test_inputs_keep_away_from_zero_and_from_symmetry():
    for n in (5, 4097):
        before, after = S.clouds(n)
        for cloud in (before, after):
            assert np.abs(cloud).min() > 1.0 and len(np.unique(cloud, axis=0)) == len(cloud)
