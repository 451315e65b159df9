"""Every case of tests/test_gpu_ransac_scale.py is what it is named for -- by the restatements alone (ransac_scale_cases.chunk_plan for
K24's launch plan, ransac_reference for draws, flags, poses and counts), no device needed.  If RANSAC_BLOCK, the number of workgroups per
CU that ransac_chunk_len asks for, or the planted recipe changes, this says which case no longer tests what it claims."""
import numpy as np
import pytest

import ransac_reference as R
import ransac_scale_cases as S
from kabsch_catalogue import posedness

BLOCK = S.RANSAC_BLOCK


def tiles_of(C):
    return -(-C // BLOCK)


def test_chunk_plan_on_shapes_worked_by_hand():
    # the planted problem (C = 1 800: 8 tiles, the last of 8 rows) on 256 CUs, as tests/test_gpu_ransac.py runs it: one tile per chunk
    for H in (4096, 512, 256, 65, 1):
        assert S.chunk_plan(H, 1800, 256) == (8, 1, 8)
    # 274 workgroups of hypotheses want ceil(512 / 274) = 2 chunks: 4 tiles each, the second one 3 full tiles and the 8 rows
    assert S.chunk_plan(70001, 1800, 256) == (2, 4, 8) and S.last_chunk_tiles(70001, 1800, 256) == 4
    assert S.chunk_plan(70001, 1800, 400) == (3, 3, 8) and S.last_chunk_tiles(70001, 1800, 400) == 2
    # 8 tiles in 5 chunks of 2: the grid has 4, not 5
    assert S.chunk_plan(256 * 103, 2048, 256) == (4, 2, 256)
    assert S.chunk_plan(1, 256, 256) == (1, 1, 256) and S.chunk_plan(1, 257, 256) == (2, 1, 1)
    # the grid's y limit
    assert S.chunk_plan(1, 256 * 70000, 40000) == (35000, 2, 256)


def test_launch_plans():
    c = S.case("many_hypotheses")
    C = len(S.pairs(c.name)[0])
    assert (C, c.hypotheses, tiles_of(C), C % BLOCK) == (1800, 70001, 8, 8)
    for cus in S.CU_COUNTS:
        chunks, per_chunk, last_rows = S.chunk_plan(c.hypotheses, C, cus)
        # fewer chunks than tiles: some workgroup takes a second trip; the last chunk ends on the 8-row tile behind a full one
        assert chunks < tiles_of(C) and per_chunk >= 2 and last_rows == 8 and S.last_chunk_tiles(c.hypotheses, C, cus) >= 2, cus
    assert c.hypotheses > 1 << 16 and c.hypotheses % BLOCK == 113

    c = S.case("unsplit")
    C = len(S.pairs(c.name)[0])
    assert (C, c.hypotheses, -(-c.hypotheses // BLOCK), c.hypotheses % BLOCK) == (600, 262145, 1025, 1) and c.hypotheses > 1 << 18
    for cus in S.CU_COUNTS:
        assert S.chunk_plan(c.hypotheses, C, cus) == (1, 3, 88), cus                 # one workgroup walks two full tiles and one of 88 rows

    for name in ("many_pairs", "many_pairs_loose"):
        c = S.case(name)
        C = len(S.pairs(name)[0])
        assert (len(c.src), C, tiles_of(C), c.hypotheses) == (140000, 126000, 493, 300)
        for cus in S.CU_COUNTS:
            chunks, per_chunk, last_rows = S.chunk_plan(c.hypotheses, C, cus)
            assert chunks < tiles_of(C) and per_chunk >= 2 and last_rows == 48, cus
    assert S.case("many_pairs").edge_similarity == 0.9 and S.case("many_pairs_loose").edge_similarity == 0.0

    # what was covered before: the planted problem at H = 4 096 on 256 CUs, one tile per chunk
    src, tgt, idx = S.planted()[:3]
    assert S.chunk_plan(4096, int((idx >= 0).sum()), 256) == (8, 1, 8)
    for name in ("offset", "no_inliers", "wrap"):
        c = S.case(name)
        print(name, S.chunk_plan(c.count, len(S.pairs(name)[0]), 256))


def test_the_cases_are_built_as_stated():
    src, tgt, idx, R0, t0, true = S.planted()
    c = S.case("many_hypotheses")
    assert c.src is src and c.tgt is tgt and c.idx is idx and (c.seed, c.edge_similarity, c.max_distance, c.first, c.count) == (7, 0.9, 0.01, 0, 70001)
    c = S.case("unsplit")
    kept = np.flatnonzero(idx >= 0)
    assert np.array_equal(np.flatnonzero(c.idx >= 0), kept[:600]) and np.array_equal(c.idx[kept[:600]], idx[kept[:600]]) and c.true.sum() >= 150
    c = S.case("many_pairs")
    n = len(c.src)
    assert c.true.sum() == 0.3 * n and (c.idx < 0).sum() == 0.1 * n and np.array_equal(c.idx[c.true], np.flatnonzero(c.true))
    # the recipe's pose and noise: every true pair within 1e-3 (and the rounding of the target to fp32) of its image under (R0, t0)
    assert np.array_equal(c.R0, R0) and np.array_equal(c.t0, t0)
    assert np.linalg.norm(c.src.astype(np.float64) @ R0.T + t0 - c.tgt, axis=1).max() <= 1e-3 + 1e-6
    c = S.case("offset")
    assert len(c.tgt) == len(c.src) + 500 == 2500 and c.idx is idx and c.idx.max() < len(c.src)
    off = np.array(S.OFFSET)
    assert np.abs(c.src - (src.astype(np.float64) + off)).max() <= np.spacing(np.float32(128)) / 2
    assert np.abs(c.tgt[:2000] - (tgt.astype(np.float64) + R0 @ off)).max() <= np.spacing(np.float32(128)) / 2
    assert np.abs(c.src.mean(axis=0)).min() > 20 and np.abs(c.tgt.mean(axis=0)).min() > 5
    c = S.case("no_inliers")
    assert len(c.src) == len(c.tgt) == 500 and np.array_equal(np.sort(c.idx), np.arange(500)) and (c.edge_similarity, c.max_distance, c.hypotheses) == (0.0, 1e-4, 512)
    c = S.case("wrap")
    assert (c.seed, c.first, c.count, c.hypotheses) == (2 ** 64 - 1, 2 ** 22 - 65, 65, 2 ** 22) and c.src is src


def test_the_wrapping_draws():
    """ranks()'s uint64 sum against draws()'s exact python integers, which are masked to 64 bits inside mix: for the `wrap` case every sum
    seed + GOLDEN (3 h + r + 1) passes 2^64 at least once before it is reduced"""
    c = S.case("wrap")
    C = len(S.pairs("wrap")[0])
    hs = range(c.first, c.first + c.count)
    assert all(c.seed + R.GOLDEN * (3 * h + r + 1) > R.MASK for h in hs for r in range(3))
    assert R.ranks(c.seed, c.first, c.count, C).tolist() == [R.draws(c.seed, h, C) for h in hs]
    # and without the wrap the same hypotheses draw something else
    assert R.ranks(0, c.first, c.count, C).tolist() != R.ranks(c.seed, c.first, c.count, C).tolist()
    i = S.pairs("wrap")[0]
    assert np.array_equal(S.restated("wrap")["triples"], i[np.array([R.draws(c.seed, h, C) for h in hs])])


@pytest.mark.parametrize("name", S.CASES)
def test_what_the_restatement_makes_of_a_case(name):
    c, ref = S.case(name), S.restated(name)
    i, s, t = S.pairs(name)
    valid, fragile = ref["valid"], ref["fragile"]
    assert len(valid) == c.count
    # hypotheses whose flag float64 does not decide: at most 0.1 %, none where the winner is pinned to the lowest valid h
    assert fragile.sum() <= (0 if name == "no_inliers" else c.count // 1000)
    assert valid.any() and ((~valid).any() or name == "many_pairs_loose")          # (no edge rule, 126 000 ranks: no repeated draw in 300)
    # the poses: at least half of them well posed (check_poses holds those entry by entry)
    cond, well, _ = posedness(ref["S"][valid], ref["g"][valid])
    assert well.sum() >= 0.5 * valid.sum()
    # the counts under the restatement's poses rounded to fp32: decided by float64 for at least 99 % of the valid hypotheses
    lo, hi = S.recount(S.restated_pose12(ref)[valid], s, t, c.max_distance)
    assert (lo == hi).mean() >= 0.99
    ties = int((hi == hi.max()).sum())
    print("%s: %d valid of %d, %d fragile, %d well posed, lo == hi for %d, best count %d shared by %d" % (
        name, valid.sum(), c.count, fragile.sum(), well.sum(), (lo == hi).sum(), hi.max(), ties))
    if name == "many_hypotheses":
        # the arg-max's tie rule is exercised: many hypotheses find all 600 true pairs and nothing else
        assert valid.sum() >= 1000 and (lo == lo.max()).sum() >= 100 and lo.max() == hi.max()
        assert np.flatnonzero(valid)[lo == lo.max()].max() > 1 << 16                  # ... some of them beyond h = 65 535
    if name == "unsplit":
        assert valid.sum() >= 1000 and np.flatnonzero(valid).max() >= (1 << 18) - BLOCK and lo.max() >= 150         # valid ones in the last full workgroup
    if name == "many_pairs":
        assert valid.sum() >= 10 and lo.max() >= 30000
    if name == "many_pairs_loose":
        assert valid.sum() >= 250 and lo.max() >= 30000
    if name == "offset":
        assert (lo >= 500).sum() >= 50
    if name == "no_inliers":
        assert hi.max() < 3                                                           # refinement is not entered whichever hypothesis wins
    if name == "wrap":
        assert valid.sum() >= 1
