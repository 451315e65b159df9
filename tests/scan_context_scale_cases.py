"""The cases of tests/test_gpu_scan_context_scale.py and what they share: the searches at which mi_scan_context_search leaves the one plan
that tests/test_gpu_scan_context.py ever takes -- one 64-row unit per chunk -- and a wide batch of descriptors.  A workgroup of K66 owns one
query and one chunk of rows; sc_chunk_len (restated here as chunk_len) asks for ceil(8 CUs / nq) chunks and clips that to the
ceil(nd / 64) units there are, so a chunk holds several units only once nq * nd is large.  The cases:

  one_chunk    7 x 13, 2500 queries, 193 rows: the whole database is one chunk of four units on any device up to 312 CUs
  chunks       20 x 60, 160 queries, 1300 rows: several chunks of several units, the last one partial, two sector tiles
  online       7 x 13, 1200 rows searched by themselves, lightly perturbed, under limit[i] = max(i - 50, 0): a trajectory's loop search
  high_rows    2 x 3, 5 queries, 2^20 + 65 rows: winners at rows 2^16 - 1, 2^16, 2^20 and the last one, in the packed key and out of it
  near_ties_*  a few thousand pairs at 20 x 60 and 7 x 13 that the full restatement can afford: duplicates at exactly equal distance and
               rows one part in a million of one component away from the winner (CPU: pruned against full; GPU: as every other case)

Each case states its plan (chunk_len, chunks, rows of the last chunk) at 32, 64, 256 and 304 CUs in PLANS, and
tests/test_scan_context_scale_cases.py holds chunk_len to every one of them.  A case is a dict: rings, sectors, query, db, limit (or
None) and what was planted.  Every case is cached, seeded and left unchanged by its users; its reference is S.search_pruned, built once.
No tolerance is introduced here."""
import functools
import time

import numpy as np

import scan_context_reference as S
from test_gpu_scan_context import cloud, random_descriptors

CHUNK = 64                           # SC_SEARCH_CHUNK (csrc/kernels.h): a chunk is a multiple of this many rows
WAVES = 2                            # SC_SEARCH_WAVES: wave w of a workgroup takes the rows begin + w, begin + w + 2, ...
SLICE = 4096                         # SC_SLICE: points of a scan per workgroup of the binning kernel
CUS = (32, 64, 256, 304)             # a partition of an MI355X, a quarter of one, the whole part, an MI300X


def frozen(a):
    a.setflags(write=False)
    return a


def chunk_len(nq, nd, cu_count):
    """sc_chunk_len (csrc/scan_context_kernels.hip) restated"""
    units = -(-nd // CHUNK)
    chunks = min(max(-(-8 * cu_count // nq), 1), units, 65535)
    return -(-units // chunks) * CHUNK


def plan(nq, nd, cu_count):
    """(chunk_len, chunks of the grid, rows of the last chunk)"""
    length = chunk_len(nq, nd, cu_count)
    chunks = -(-nd // length)
    return length, chunks, nd - (chunks - 1) * length


# what every case claims, by CU count: (chunk_len, chunks, rows of the last chunk)
PLANS = {
    # ceil(8 CUs / 2500) = 1 chunk up to 312 CUs: four units, the last of which holds one row
    "one_chunk": {32: (256, 1, 193), 64: (256, 1, 193), 256: (256, 1, 193), 304: (256, 1, 193)},
    # 21 units.  256 CUs: 13 chunks wanted, two units each, so 11 chunks of 128 rows, the last of 20; 304 CUs: 16 wanted, the same chunks;
    # 64 CUs: 4 chunks of six units, the last of 148 rows; 32 CUs: 2 chunks of eleven units, 704 and 596 rows
    "chunks": {32: (704, 2, 596), 64: (384, 4, 148), 256: (128, 11, 20), 304: (128, 11, 20)},
    # 19 units.  256 CUs: 2 chunks of ten units, 640 and 560 rows; 304 CUs: 3 chunks of seven units, the last of 304 rows; up to 150 CUs
    # one chunk of all 19
    "online": {32: (1216, 1, 1200), 64: (1216, 1, 1200), 256: (640, 2, 560), 304: (448, 3, 304)},
    # 16 386 units, ceil(8 CUs / 5) chunks wanted: 52, 103, 410 and 487 chunks of 316, 160, 40 and 34 units
    "high_rows": {32: (20224, 52, 17217), 64: (10240, 103, 4161), 256: (2560, 410, 1601), 304: (2176, 482, 1985)},
    "near_ties_20x60": {32: (64, 4, 8), 64: (64, 4, 8), 256: (64, 4, 8), 304: (64, 4, 8)},
    "near_ties_7x13": {32: (64, 2, 36), 64: (64, 2, 36), 256: (64, 2, 36), 304: (64, 2, 36)},
}


def rolled(row, k, noise_seed=None, sectors_axis=-1):
    """a descriptor seen again turned by k sectors; noise_seed: with 5 % of something else on top"""
    out = np.roll(row, k, axis=sectors_axis)
    if noise_seed is not None:
        out = out + random_descriptors(noise_seed, 1, *row.shape, empty=0.0)[0] * np.float32(0.05)
    return out.astype(np.float32)


def case(rings, sectors, query, db, limit=None, **planted):
    return dict(rings=rings, sectors=sectors, query=frozen(np.ascontiguousarray(query, np.float32)), db=frozen(np.ascontiguousarray(db, np.float32)),
                limit=None if limit is None else frozen(np.ascontiguousarray(limit, np.int32)), **planted)


# ---- 1. one chunk, many units, any device
@functools.lru_cache(maxsize=None)
def one_chunk():
    """Queries 0, 1250 and 2499 are rows 0, 64 and 192 -- the first row of the first two units and the one row of the fourth -- turned by
    3, 5 and 11 sectors; all others are random."""
    db = random_descriptors(6601, 3 * CHUNK + 1, 7, 13)
    query = random_descriptors(6602, 2500, 7, 13)
    at, rows, turns = [0, 1250, 2499], [0, 64, 192], [3, 5, 11]
    for q, r, k in zip(at, rows, turns):
        query[q] = rolled(db[r], k)
    return case(7, 13, query, db, at=at, rows=rows, turns=turns)


# ---- 2. several chunks of several units
CHUNKS_DUPLICATES = (5, 700, 1290)   # one descriptor in three rows: chunks 0, 5 and 10 of 128 rows
# winners by construction: the first and the last row of a chunk of 128 (and of 384 and of 704) rows, rows of either parity -- of either
# wave --, the first row of the partial last chunk and the database's last row
CHUNKS_WINNERS = (384, 511, 127, 128, 703, 704, 1151, 1152, 1280, 1299, 777, 64)


@functools.lru_cache(maxsize=None)
def chunks():
    """Query 0 is the duplicated descriptor turned by 9 sectors: the lowest of its three rows wins and second == dist.  Queries 1 .. 12 are
    the rows of CHUNKS_WINNERS turned by 1, 6, 11, ... sectors, every other one with 5 % of noise on top.  The other 147 are random."""
    db = random_descriptors(6611, 1300, 20, 60)
    for r in CHUNKS_DUPLICATES[1:]:
        db[r] = db[CHUNKS_DUPLICATES[0]]
    query = random_descriptors(6612, 160, 20, 60)
    query[0] = rolled(db[CHUNKS_DUPLICATES[0]], 9)
    turns = [(1 + 5 * i) % 60 for i in range(len(CHUNKS_WINNERS))]
    for i, (r, k) in enumerate(zip(CHUNKS_WINNERS, turns)):
        query[1 + i] = rolled(db[r], k, noise_seed=6620 + i if i % 2 else None)
    return case(20, 60, query, db, turns=turns)


# ---- 3. the online shape
ONLINE_ROWS, ONLINE_WINDOW, ONLINE_BACK = 1200, 50, 200
ONLINE_REVISITS = tuple(range(250, ONLINE_ROWS, 37))         # 26 rows; none of them is the earlier row of another


@functools.lru_cache(maxsize=None)
def online():
    """Row i of ONLINE_REVISITS is row i - 200 turned by a few sectors: a place seen again.  Query i is row i with every bin within 1 % of
    its value, and sees the rows below i - 50: not itself, so most queries find some row or other, and a revisit finds its place.  The
    first 51 queries see no row, query 51 sees one."""
    db = random_descriptors(6631, ONLINE_ROWS, 7, 13)
    turns = [1 + i % 12 for i in range(len(ONLINE_REVISITS))]
    for i, k in zip(ONLINE_REVISITS, turns):
        db[i] = rolled(db[i - ONLINE_BACK], k)
    rng = np.random.default_rng(6632)
    query = (db * rng.uniform(0.99, 1.01, db.shape)).astype(np.float32)
    limit = np.maximum(np.arange(ONLINE_ROWS) - ONLINE_WINDOW, 0)
    return case(7, 13, query, db, limit=limit, turns=turns)


# ---- 4. rows beyond 2^16 and 2^20
HIGH_ROWS = (1 << 20) + 65
HIGH_PLANTED = ((1 << 16) - 1, 1 << 16, 1 << 20, (1 << 20) + 64, 7)       # where query i's copy lies; the last one lies at 2^20 + 1 as well
HIGH_TWICE = (1 << 20) + 1


@functools.lru_cache(maxsize=None)
def high_rows():
    """The recipe's rows with 1 added to every bin, so that no column is empty: with three columns of two rings a row that has one or two
    columns left meets any query to within fp32 rounding through those alone (a million rows hold every angle to one part in 10^6), and
    the lowest such row would win every search.  With three full columns the nearest random row lies some 10^-5 away.  The queries are
    five random descriptors of that kind, and their copies, turned by 0 to 2 sectors, lie at HIGH_PLANTED."""
    db = random_descriptors(6641, HIGH_ROWS, 2, 3, empty=0.0) + np.float32(1.0)
    query = random_descriptors(6642, 5, 2, 3, empty=0.0) + np.float32(1.0)
    turns = [1, 2, 1, 0, 2]
    for q, r, k in zip(query, HIGH_PLANTED, turns):
        db[r] = rolled(q, -k)
    db[HIGH_TWICE] = db[HIGH_PLANTED[4]]
    return case(2, 3, query, db, turns=turns)


# ---- 5. near ties, at sizes the full restatement affords
def near_ties(rings, sectors, nq, nd, seed):
    """Query 0: a descriptor that two rows hold, the lowest wins and second == dist.  Queries 1 and 2: a row that has a twin with one bin
    one part in a million larger, the twin below it (query 1) and above it (query 2): what separates the two is below the twin
    restatement's resolution, so the pruning has to keep both.  Query 3: two rows hold the same noisy copy of its winner and tie as the runner-up."""
    db = random_descriptors(seed, nd, rings, sectors)
    query = random_descriptors(seed + 1, nq, rings, sectors)
    dup, above, below, third = (nd // 3, nd - 2), (nd // 2, 4), (9, nd - 5), (nd // 4, 2, nd - 1)
    db[dup[1]] = db[dup[0]]
    for own, twin in (above, below):
        db[twin] = db[own]
        r, s = np.argwhere(db[own] > 0)[own % 7]
        db[twin, r, s] = np.float32(float(db[own, r, s]) * (1.0 + 1e-6))
        assert db[twin, r, s] != db[own, r, s]
    db[third[1]] = db[third[2]] = rolled(db[third[0]], 0, noise_seed=seed + 2)
    query[0], query[1], query[2] = rolled(db[dup[0]], 3), rolled(db[above[0]], 5), rolled(db[below[0]], sectors - 1)
    query[3] = rolled(db[third[0]], 2)
    return case(rings, sectors, query, db, dup=dup, above=above, below=below, third=third)


@functools.lru_cache(maxsize=None)
def near_ties_20x60():
    return near_ties(20, 60, 12, 200, 6651)          # 2 400 pairs


@functools.lru_cache(maxsize=None)
def near_ties_7x13():
    return near_ties(7, 13, 40, 100, 6661)           # 4 000 pairs


CASES = {"one_chunk": one_chunk, "chunks": chunks, "online": online, "high_rows": high_rows, "near_ties_20x60": near_ties_20x60,
         "near_ties_7x13": near_ties_7x13}
SCALE = ("one_chunk", "chunks", "online", "high_rows")
REFERENCE_SECONDS, REFERENCE_STATS = {}, {}        # by name: what tests/test_scan_context_scale_cases.py prints


@functools.lru_cache(maxsize=None)
def reference(name):
    """(idx, dist, shift, second) of a case by S.search_pruned, computed once and frozen"""
    c = CASES[name]()
    stats = {}
    t0 = time.perf_counter()
    out = tuple(frozen(a) for a in S.search_pruned(c["query"], c["db"], c["limit"], stats=stats))
    REFERENCE_SECONDS[name], REFERENCE_STATS[name] = time.perf_counter() - t0, stats
    return out


# ---- 6. the search cases of tests/test_gpu_scan_context.py, input for input, for the comparison of search_pruned with search on the CPU
def existing_search_cases(planted_case):
    """(label, query, db, limit) of every search that tests/test_gpu_scan_context.py runs; planted_case: planted(capi) of
    tests/test_scan_context_reference.py"""
    from test_scan_context_reference import SHAPES
    query = random_descriptors(1, 1, 20, 60)
    for nd in (1, 63, 64, 65, 2 * CHUNK + 1, 300):                       # test_search_database_sizes
        db = random_descriptors(1000 + nd, nd, 20, 60)
        db[nd // 2] = query[0]
        yield "nd %d" % nd, query, db, None
    db = random_descriptors(5, 2 * CHUNK + 1, 7, 13)                     # test_search_query_counts
    for nq in (1, 5, 70):
        yield "nq %d" % nq, random_descriptors(50 + nq, nq, 7, 13), db, None
    for rings, sectors in SHAPES:                                        # test_search_shapes
        db = random_descriptors(10 * rings + sectors, 70, rings, sectors)
        query = (np.roll(db[[3, 41, 69]], sectors // 2, axis=2) + random_descriptors(7, 3, rings, sectors, empty=0.0) * np.float32(0.05)).astype(np.float32)
        yield "%d x %d" % (rings, sectors), query, db, None
    db = random_descriptors(21, 80, 20, 60)                              # test_search_contract_cases
    db[:, :, ::2] = 0
    db[17] = 0
    db[60] = db[30]
    query = np.stack([db[30], np.zeros((20, 60), np.float32), np.roll(db[75], 7, axis=1), db[17]])
    yield "contract", query, db, None
    yield "an all-empty row alone", query[:1], db[17:18], None
    for limit in ([0, 0, 0, 0], [1, 1, 1, 1], [80, 80, 80, 80], [0, 1, 80, 31], [-5, 64, 65, 30]):
        yield "limit %s" % limit, query, db, np.array(limit, np.int32)
    yield "planted", planted_case[6], planted_case[5], None              # test_planted_places_end_to_end


# ---- 7. descriptors in a wide batch
BATCH_SCANS, BATCH_SIZES, BATCH_LONG_AT = 300, (0, 1, 63, 200, 700), 137
BATCH_SAMPLED = (0, 1, 2, 59, 136, 137, 138, 211, 298, 299)              # each against its own single-scan call


@functools.lru_cache(maxsize=None)
def batch():
    """(clouds, centres): 300 scans of 0, 1, 63, 200 or 700 points, scan 137 of SC_SLICE + 1 -- the batch's grid is two slices deep for
    one scan and for no other --, every scan about a centre of its own"""
    rng = np.random.default_rng(6671)
    sizes = rng.choice(BATCH_SIZES, BATCH_SCANS)
    sizes[:5] = BATCH_SIZES                                              # every size is there, an empty scan first
    sizes[BATCH_LONG_AT] = SLICE + 1
    clouds = []
    centres = (rng.uniform(-20, 20, (BATCH_SCANS, 3)) * [1.0, 1.0, 0.05]).astype(np.float32)      # the heights stay on both sides of -z_offset
    for i, n in enumerate(sizes):
        clouds.append(frozen((cloud(6700 + i, int(n)) + centres[i]).astype(np.float32)))
    return tuple(clouds), frozen(centres)
