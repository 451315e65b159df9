"""CPU suite: the restated contract of tests/ransac_reference.py -- the splitmix64 draws against values worked out by hand, the ranks'
uniformity, the edge rule and the count rule on hand cases, and the planted problem of the GPU suite checked with the restatement alone."""
import numpy as np

import ransac_reference as R


def test_draws_against_hand_computed_values():
    # u_r of hypotheses 0 and 5, worked out step by step with 64-bit integers, for two seeds
    assert [R.mix(0 + R.GOLDEN * k) for k in (1, 2, 3)] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    assert [R.mix(0 + R.GOLDEN * k) for k in (16, 17, 18)] == [0x84BB3F97971D80AB, 0x7D29825C75521255, 0xC3CF17102B7F7F86]
    seed = 0xDEADBEEF12345678
    assert [R.mix(seed + R.GOLDEN * k) for k in (1, 2, 3)] == [0x4DC32B44ABDC6395, 0xB37AFA501D2539C9, 0x2C9C40E31313E214]
    assert R.draws(0, 0, 1000) == [883, 431, 26] and R.draws(0, 5, 1000) == [518, 488, 764]
    assert R.draws(seed, 0, 1000) == [303, 701, 174] and R.draws(seed, 5, 1000) == [709, 53, 38]
    # rank = floor(top 32 bits * C / 2^32): 0xE220A839 * 1000 >> 32
    assert (0xE220A839 * 1000) >> 32 == 883
    for s in (0, seed, (1 << 64) - 1):
        assert R.ranks(s, 3, 40, 77).tolist() == [R.draws(s, h, 77) for h in range(3, 43)]


def test_ranks_are_uniform():
    # 1e5 draws into 50 buckets: every bucket within 5 sigma of its binomial mean (sigma = sqrt(N p (1 - p)) = 44.3)
    rk = R.ranks(12345, 0, 100000 // 3 + 1, 50).ravel()[:100000]
    counts = np.bincount(rk, minlength=50)
    assert rk.min() == 0 and rk.max() == 49 and (np.abs(counts - 2000) <= 5 * np.sqrt(100000 * 0.02 * 0.98)).all()
    assert rk[:10].tolist() != R.ranks(12346, 0, 4, 50).ravel()[:10].tolist()


def test_edge_rule_on_hand_cases():
    tri = np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]], np.float64)
    for scale, e, want in ((1.0, 0.9, True), (0.91, 0.9, True), (1 / 0.91, 0.9, True), (0.89, 0.9, False), (1 / 0.89, 0.9, False), (0.1, 0.0, True), (0.51, 0.5, True), (0.49, 0.5, False)):
        ok, fragile = R.edge_rule(tri, tri * scale, e)
        assert ok[0] == want and not fragile[0], (scale, e)
    ok, fragile = R.edge_rule(tri, tri * 0.5, 0.5)        # exactly on the threshold: lt2 = 0.25 ls2 = e2 ls2
    assert ok[0] and fragile[0]
    stretched = tri.copy()
    stretched[0, 2] = [0, 2, 0]                           # one edge doubled: that pair fails
    assert not R.edge_rule(tri, stretched, 0.9)[0][0]


def test_count_rule_on_hand_cases():
    s = np.array([[1, 2, 3], [0, 0, 0], [1, 0, 0], [0, 0, 1]], np.float64)
    # R = rotation by 90 degrees about z (x -> y), column-major; t = (10, 20, 30)
    pose = np.array([[0, 1, 0, -1, 0, 0, 0, 0, 1, 10, 20, 30]], np.float32)
    image = np.array([[8, 21, 33], [10, 20, 30], [10, 21, 30], [10, 20, 31]], np.float64)
    t = image + np.array([[0.5, 0, 0], [0, 0.5, 0], [0, 0, 0.5000001], [0.3, 0.4, 0]])
    lo, hi, d2 = R.count_rule(pose, s, t, 0.5)
    assert np.allclose(d2[0], [0.25, 0.25, 0.25000010000001, 0.25]) and lo[0] <= 3 <= hi[0]
    lo, hi, _ = R.count_rule(pose, s, t, 0.51)
    assert lo[0] == hi[0] == 4
    lo, hi, _ = R.count_rule(pose, s, t, 0.49)
    assert lo[0] == hi[0] == 0


def test_the_planted_problem_is_what_the_gpu_suite_relies_on():
    src, tgt, idx, R0, t0, true = R.planted()
    assert true.sum() == 600 and (idx < 0).sum() == 200
    hy = R.hypotheses(src, tgt, idx, 7, 0, 4096, 0.9)
    i, s, t = R.correspondences(src, tgt, idx)
    assert hy["fragile"].sum() <= 4                       # at most 0.1 % of 4 096
    pose = np.concatenate([hy["R64"].transpose(0, 2, 1).reshape(-1, 9), hy["t64"]], axis=1).astype(np.float32)
    lo, hi, d2 = R.count_rule(pose[hy["valid"]], s, t, 0.01)
    assert (lo >= 500).sum() >= 50
    # the restatement's own winner, refined once in float64 over its inliers, explains every true pair and is within max_distance everywhere
    w = int(np.argmax(lo))
    inl = d2[w] <= 1e-4
    Rw, tw = R.kabsch_pairs64(s[inl], t[inl])
    assert (np.linalg.norm(s @ Rw.T + tw - t, axis=1)[true[i]] <= 0.01).all()
    assert np.linalg.norm(src.astype(np.float64) @ Rw.T + tw - (src.astype(np.float64) @ R0.T + t0), axis=1).max() <= 0.01
