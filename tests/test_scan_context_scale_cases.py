"""CPU suite: S.search_pruned, the restatement that tests/test_gpu_scan_context_scale.py compares with, held to S.search bit for bit wherever
S.search is affordable -- every search of tests/test_gpu_scan_context.py, the near-tie cases of a few thousand pairs, the million rows of
2 x 3 -- its bound e_bound held against the restatement's own fp32 distances (never against a device), and every case of
tests/scan_context_scale_cases.py held to what it claims: its plan at 32, 64, 256 and 304 CUs by a restatement of sc_chunk_len, its planted
winners, the limits of the online case.

Reference build times, one BLAS thread, on the CPU this was written on: one_chunk 1.6 s, chunks 6.2 s, online 2.9 s, high_rows 1.7 s (its
full S.search: 6 s), near_ties_20x60 and near_ties_7x13 0.2 s and less (their full S.search: 2.5 s and 0.2 s).  They are printed with each
case, and a case that took 20 s would fail."""
import numpy as np
import pytest

import scan_context_reference as S
import scan_context_scale_cases as K
from test_scan_context_reference import planted


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_outputs(got, want):
    return (all(a.dtype == b.dtype and a.shape == b.shape for a, b in zip(got, want)) and np.array_equal(got[0], want[0])
            and np.array_equal(got[2], want[2]) and np.array_equal(bits(got[1]), bits(want[1])) and np.array_equal(bits(got[3]), bits(want[3])))


def describe(name):
    ref = K.reference(name)
    c, stats = K.CASES[name](), K.REFERENCE_STATS[name]
    e = S.e_bound(c["rings"])
    print("%-16s %d x %d, nq %d, nd %d: reference %.1f s, rows kept per query %.2f on average and %d at the most, worst |fp32 - twin| %.3g (e = %.3g)"
          % (name, c["rings"], c["sectors"], len(c["query"]), len(c["db"]), K.REFERENCE_SECONDS[name], stats["kept"].mean(), stats["kept"].max(), stats["worst"], e))
    assert K.REFERENCE_SECONDS[name] < 20.0
    assert stats["worst"] < e
    return c, ref


# ---- 1. the plan
def test_the_constants_are_the_kernels(capi):
    assert (K.CHUNK, K.WAVES, K.SLICE) == (capi.SC_SEARCH_CHUNK, capi.SC_SEARCH_WAVES, capi.SC_SLICE)


def test_chunk_len_by_hand():
    # the existing suite's sizes: one unit per chunk on every device from 32 CUs on
    for nq, nd in ((1, 300), (70, 129), (3, 70), (4, 80), (40, 40)):
        for cus in K.CUS:
            assert K.chunk_len(nq, nd, cus) == K.CHUNK, (nq, nd, cus)
    assert K.chunk_len(1, 1, 256) == 64 and K.chunk_len(1, 10 ** 4, 256) == 64 and K.chunk_len(100, 10 ** 4, 256) == 512
    assert K.chunk_len(1, 1 << 26, 256) == 512 * 64                    # 2^20 units over 2048 chunks
    assert K.chunk_len(1, 1 << 26, 10 ** 4) == 17 * 64                  # grid.y: 65 535 chunks at the most


@pytest.mark.parametrize("name", sorted(K.CASES))
def test_every_case_takes_the_plan_it_claims(name):
    c = K.CASES[name]()
    nq, nd = len(c["query"]), len(c["db"])
    assert set(K.PLANS[name]) == set(K.CUS)
    for cus in K.CUS:
        assert K.plan(nq, nd, cus) == K.PLANS[name][cus], (name, cus)
        length, chunks, last = K.plan(nq, nd, cus)
        assert length % K.CHUNK == 0 and 0 < last <= length and (chunks - 1) * length + last == nd
    if name in K.SCALE:                                                  # several units per chunk on every device; several chunks where claimed
        assert all(K.PLANS[name][cus][0] > K.CHUNK for cus in K.CUS)
    if name in ("chunks", "online"):
        assert K.PLANS[name][256][1] > 1 and K.PLANS[name][304][1] > 1
    if name == "one_chunk":                                              # ... up to 312 CUs and no further
        assert K.plan(nq, nd, 312) == (256, 1, 193) and K.plan(nq, nd, 313)[1] == 2


# ---- 2. pruned against full
def test_pruned_equals_full_on_every_search_of_the_first_suite(capi):
    labels = []
    for label, query, db, limit in K.existing_search_cases(planted(capi)):
        stats = {}
        got = S.search_pruned(query, db, limit, stats=stats)
        assert same_outputs(got, S.search(query, db, limit)), label
        assert stats["worst"] < S.e_bound(query.shape[1]), label
        labels.append(label)
    assert len(labels) == 6 + 3 + 4 + 2 + 5 + 1


@pytest.mark.parametrize("name", ["near_ties_20x60", "near_ties_7x13"])
def test_pruned_equals_full_on_near_ties(name):
    c, ref = describe(name)
    full = S.search(c["query"], c["db"])
    assert same_outputs(ref, full)
    idx, dist, shift, second = ref
    sectors, e = c["sectors"], S.e_bound(c["rings"])
    assert idx[0] == c["dup"][0] and shift[0] == sectors - 3 and bits(second[:1]) == bits(dist[:1])          # the duplicate, at exactly the distance
    for q, (own, twin), turn in ((1, c["above"], 5), (2, c["below"], sectors - 1)):
        assert idx[q] in (own, twin) and shift[q] == sectors - turn and abs(float(second[q]) - float(dist[q])) <= 2 * e
    assert idx[3] == c["third"][0] and second[3] > dist[3] + 4 * e
    # the bound, on every row and not on the kept ones alone: the restatement's fp32 minimum of a row against the twin's
    uq, mq = S.unit_columns(c["query"])
    uc, mc = S.unit_columns(c["db"])
    twin_rows = S.row_minima_twin(c["query"], c["db"])
    worst = 0.0
    for i in range(0, len(uq), 3 if c["rings"] == 20 else 1):
        d32 = S.shift_distances(uq[i], mq[i], uc, mc).min(axis=1).astype(np.float64)
        worst = max(worst, float(np.abs(d32 - twin_rows[i]).max()))
        assert np.abs(S.shift_distances_twin(c["query"][i], c["db"]).min(axis=1) - twin_rows[i]).max() < 2.0 ** -45       # the two twins are one
    print("%s: worst |fp32 - twin| over all rows %.3g, e = %.3g" % (name, worst, e))
    assert worst < e


def test_pruned_equals_full_on_a_million_rows():
    c, ref = describe("high_rows")
    assert same_outputs(ref, S.search(c["query"], c["db"]))
    idx, dist, shift, second = ref
    assert idx.tolist() == list(K.HIGH_PLANTED) and len(c["db"]) == K.HIGH_ROWS == (1 << 20) + 65
    assert idx[3] == K.HIGH_ROWS - 1 and shift.tolist() == [(3 - k) % 3 for k in c["turns"]]
    assert np.array_equal(c["db"][K.HIGH_TWICE], c["db"][7]) and bits(second[4:]) == bits(dist[4:]) and (second[:4] > dist[:4]).all()
    assert (np.abs(dist) <= S.e_bound(2)).all()


# ---- 3. the scale cases are what they are named for
def test_one_chunk_finds_its_planted_rows():
    c, (idx, dist, shift, second) = describe("one_chunk")
    assert (len(c["query"]), len(c["db"])) == (2500, 3 * K.CHUNK + 1)
    assert idx[c["at"]].tolist() == c["rows"] == [0, 64, 192] and shift[c["at"]].tolist() == [13 - k for k in c["turns"]]
    assert (np.abs(dist[c["at"]]) <= S.e_bound(7)).all() and (second > dist).all()
    assert len(np.unique(idx // K.CHUNK)) == 4 and len(np.unique(idx % K.WAVES)) == 2        # winners in every unit and from either wave


def test_chunks_finds_its_planted_rows():
    c, (idx, dist, shift, second) = describe("chunks")
    assert (len(c["query"]), len(c["db"])) == (160, 1300)
    assert idx[0] == K.CHUNKS_DUPLICATES[0] and shift[0] == 60 - 9 and bits(second[:1]) == bits(dist[:1])
    assert len({r // 128 for r in K.CHUNKS_DUPLICATES}) == 3                                  # three chunks at 256 and 304 CUs
    n = len(K.CHUNKS_WINNERS)
    assert idx[1:1 + n].tolist() == list(K.CHUNKS_WINNERS) and shift[1:1 + n].tolist() == [(60 - k) % 60 for k in c["turns"]]
    assert (second[1:1 + n] > dist[1:1 + n]).all()
    for length in (128, 384, 704):                                                            # a chunk's first and last row, of either parity
        assert {0, length - 1} <= {r % length for r in K.CHUNKS_WINNERS}
    assert 1280 in K.CHUNKS_WINNERS and 1299 in K.CHUNKS_WINNERS
    assert len(np.unique(idx // 128)) == 11 and len(np.unique(idx % K.WAVES)) == 2           # winners in every chunk of the plan at 256 CUs


def test_online_is_a_trajectory_under_its_limits():
    c, (idx, dist, shift, second) = describe("online")
    limit = c["limit"]
    n, window = K.ONLINE_ROWS, K.ONLINE_WINDOW
    assert len(c["query"]) == len(c["db"]) == n and np.array_equal(limit, np.maximum(np.arange(n) - window, 0))
    none = slice(0, window + 1)
    assert (idx[none] == -1).all() and np.isinf(dist[none]).all() and (shift[none] == 0).all() and np.isinf(second[none]).all()
    assert limit[window + 1] == 1 and idx[window + 1] == 0 and np.isinf(second[window + 1]) and np.isfinite(second[window + 2:]).all()
    seen = np.arange(n) > window
    assert (idx[seen] >= 0).all() and (idx[seen] < limit[seen]).all()
    # at 256 CUs: two chunks of 640 rows.  Every limit from 1 to 1149 ends inside a chunk; the second chunk is cut off whole up to query 690
    length = K.PLANS["online"][256][0]
    assert length == 640 and (limit[seen] % length != 0).sum() >= len(limit[seen]) - 1 and (limit <= length).sum() == 691
    revisits = np.array(K.ONLINE_REVISITS)
    assert len(revisits) == 26 and not set(revisits) & set(revisits - K.ONLINE_BACK)
    assert np.array_equal(idx[revisits], revisits - K.ONLINE_BACK) and shift[revisits].tolist() == [13 - k for k in c["turns"]]
    assert (dist[revisits] < 1e-3).all() and (second[revisits] > 0.05).all()
    # winners in the second chunk while the limit ends in it, and revisits whose place lies in the first chunk under a limit in the second
    assert (idx >= length).any() and ((revisits - K.ONLINE_BACK < length) & (limit[revisits] > length)).sum() >= 3


def test_the_batch_is_what_it_claims(capi):
    clouds, centres = K.batch()
    sizes = np.array([len(c) for c in clouds])
    assert len(clouds) == K.BATCH_SCANS == 300 and centres.shape == (300, 3)
    assert set(sizes) == set(K.BATCH_SIZES) | {capi.SC_SLICE + 1} and (sizes == capi.SC_SLICE + 1).sum() == 1 and sizes[K.BATCH_LONG_AT] == capi.SC_SLICE + 1
    assert sizes[0] == 0 and all((sizes == s).sum() >= 20 for s in K.BATCH_SIZES)
    assert len(set(K.BATCH_SAMPLED)) == 10 and K.BATCH_LONG_AT in K.BATCH_SAMPLED and 0 in {sizes[i] for i in K.BATCH_SAMPLED}
