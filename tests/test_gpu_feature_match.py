"""GPU suite of mi_feature_match against the restatement of tests/match_reference.py, which emulates the contract's fp32 fmaf chain bit for
bit.  Every reference is built once (lru_cache), left unchanged, and shared by the tests that need it.

The bounds (none of them taken from what the device gives):
  idx   equal to the restatement's, with and without the mutual filter -- the chain is emulated exactly, so there is no fragile case
  d2    |got - float64| <= 2^-23 float64: one fp32 rounding, 2^-24, doubled (the float64 sum of at most 64 terms adds 1e-14); +inf at -1

The shapes follow the kernel's tiling (match_kernels.hip): 32 queries per wave, 128 per workgroup, targets in tiles of 128 split into
subtiles of 32, k-steps of 2, one kernel instantiation each for dim <= 16, <= 34, <= 64, and chunks of whole tiles merged by atomicMin
(as many chunks as it takes to give two workgroups per CU, at most one per tile)."""
import functools

import numpy as np
import pytest

import match_reference as M

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257)
DIMS = (1, 2, 3, 15, 16, 17, 32, 33, 34, 35, 63, 64)


def frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def rows(kind, n, dim, seed):
    rng = np.random.default_rng([seed, n, dim])
    if kind == "fpfh_range":
        a = rng.uniform(0, 200, (n, dim))
    elif kind == "mixed_sign":                        # the keys are negative wherever 2 q.t > |t|^2
        a = rng.normal(size=(n, dim)) * rng.choice([0.01, 1.0, 30.0], (n, 1))
    elif kind == "ties":                              # small integers: many exact ties between different targets
        a = rng.integers(-2, 3, (n, dim)).astype(np.float64)
    else:                                             # "lattice": ties, exact hits and negative keys at once
        a = rng.integers(-20, 21, (n, dim)).astype(np.float64)
    return frozen(np.ascontiguousarray(a, np.float32))


@functools.lru_cache(maxsize=None)
def case(kind, n, m, dim):
    q, t = rows(kind, n, dim, 1), rows(kind, m, dim, 2)
    both = M.directions(q, t)
    plain, mutual = M.match(q, t, both=both), M.match(q, t, mutual=True, both=both)
    return q, t, tuple(frozen(a) for a in plain), tuple(frozen(a) for a in mutual)


def check(ctx, q, t, plain, mutual, what):
    for want, flag in ((plain, False), (mutual, True)):
        idx, d2 = ctx.feature_match(q, t, mutual=flag, want_d2=True)
        assert np.array_equal(idx, want[0]), "%s mutual %d: %d of %d matches differ" % (what, flag, (idx != want[0]).sum(), len(idx))
        kept, ref = M.d2_float64(q, t, want[0])
        assert np.isposinf(d2[~kept]).all() and (np.abs(d2[kept].astype(np.float64) - ref) <= 2.0 ** -23 * ref).all(), what
        assert np.array_equal(ctx.feature_match(q, t, mutual=flag), want[0]), what        # d2 == NULL
    return idx, d2


# ---- 1. sizes around the tiles, dims around the k-step and the three instantiations
@pytest.mark.parametrize("s", SIZES)
def test_sizes_around_the_tiles(ctx, s):
    for n, m in ((s, 257), (257, s), (s, s)):
        for kind in ("fpfh_range", "ties"):
            q, t, plain, mutual = case(kind, n, m, 33)
            check(ctx, q, t, plain, mutual, "%s %d x %d" % (kind, n, m))


@pytest.mark.parametrize("dim", DIMS)
def test_dims_around_the_k_step(ctx, dim):
    for kind in ("mixed_sign", "ties"):
        q, t, plain, mutual = case(kind, 65, 257, dim)
        check(ctx, q, t, plain, mutual, "%s dim %d" % (kind, dim))
    q, t, plain, mutual = case("mixed_sign", 65, 257, dim)
    h, _ = M.keys(q, t)
    assert dim < 3 or (h.min(axis=1) < 0).any()       # the winning keys are negative: the ordered mapping is exercised


def test_fifteen_hundred_against_two_thousand(ctx):
    q, t, plain, mutual = case("fpfh_range", 1500, 2000, 33)       # 12 workgroups of queries x (from 43 CUs on) 16 chunks of one tile
    check(ctx, q, t, plain, mutual, "1500 x 2000")
    assert (mutual[0] >= 0).any() and (mutual[0] < 0).any()


def test_chunks_of_several_tiles(ctx):
    # 41 workgroups of queries and 15 tiles of targets: match_chunk_len wants ceil(2 CUs / 41) chunks, fewer than the 15 tiles on any device of
    # up to 307 CUs, so a chunk holds several tiles whatever the part or its partition (256 CUs: 13 wanted, chunks of two tiles, the last
    # one of one and a part; 32 CUs: two chunks of eight and seven)
    # integer rows in [-20, 20]^2: 1681 distinct rows among 1800 targets, so there are exact hits, duplicates in different chunks and ties
    q, t, plain, mutual = case("lattice", 5200, 1800, 2)
    check(ctx, q, t, plain, mutual, "5200 x 1800")


# ---- 2. constructed data
def test_duplicates_and_exact_hits(ctx):
    q, t = (np.array(a) for a in case("fpfh_range", 129, 257, 33)[:2])
    t[200], t[140], t[37] = t[5], t[5], t[5]          # duplicates across subtiles and tiles
    q[0], q[64], q[128] = t[200], t[140], t[256]
    idx, d2 = check(ctx, q, t, M.match(q, t), M.match(q, t, mutual=True), "duplicates")
    idx, d2 = ctx.feature_match(q, t, want_d2=True)
    assert idx[0] == 5 and idx[64] == 5 and idx[128] == 256 and d2[0] == 0 and d2[64] == 0 and d2[128] == 0
    midx = ctx.feature_match(q, t, mutual=True)
    assert midx[0] == 5 and midx[64] == -1 and midx[128] == 256    # two queries at one target at equal distance: the lower query


def test_two_queries_sharing_a_target_keep_the_nearer(ctx):
    t = np.zeros((3, 33), np.float32)
    t[1, 0], t[2, 1] = 100, 100
    q = np.zeros((3, 33), np.float32)
    q[0, 0], q[1, 0], q[2, 1] = 90, 97, 60            # queries 0 and 1 both match target 1; query 1 is nearer
    idx, d2 = ctx.feature_match(q, t, want_d2=True)
    assert idx.tolist() == [1, 1, 2] and d2.tolist() == [100.0, 9.0, 1600.0]
    midx, md2 = ctx.feature_match(q, t, mutual=True, want_d2=True)
    assert midx.tolist() == [-1, 1, 2] and md2.tolist() == [np.inf, 9.0, 1600.0]
    assert np.array_equal(midx, M.match(q, t, mutual=True)[0])


@functools.lru_cache(maxsize=None)
def fpfh_pair_clouds():
    """The `sphere` cloud of tests/test_gpu_fpfh.py's recipe (a noisy unit sphere of 2000 points, normals with noise of 0.05) and a
    rotated copy of it in another order."""
    rng = np.random.default_rng(71)
    unit = lambda v: v / np.linalg.norm(v, axis=1, keepdims=True)
    d = unit(rng.normal(size=(2000, 3)))
    p, nr = d * (1 + 0.01 * rng.normal(size=2000))[:, None], unit(d + 0.05 * rng.normal(size=(2000, 3)))
    a = np.deg2rad(40.0)
    R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]) @ np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    perm = rng.permutation(2000)
    f = lambda x: frozen(np.ascontiguousarray(x, np.float32))
    return f(p), f(nr), f((p @ R.T)[perm]), f((nr @ R.T)[perm]), perm


def test_a_real_fpfh_pair(ctx):
    """Measured on an MI355X: all 2000 points are kept by the mutual filter and every one of them is matched to its own image (the
    descriptors of a rotated copy differ by rounding only).  Printed, not asserted: the assertion is the equality with the restatement."""
    p, nr, p2, nr2, perm = fpfh_pair_clouds()
    fa, fb = ctx.fpfh_features(p, nr, 16), ctx.fpfh_features(p2, nr2, 16)
    both = M.directions(fb, fa)
    idx, d2 = check(ctx, fb, fa, M.match(fb, fa, both=both), M.match(fb, fa, mutual=True, both=both), "fpfh")
    kept = idx >= 0
    print("fpfh pair: %d of 2000 mutual matches kept, %d of them the point itself" % (kept.sum(), (perm[kept] == idx[kept]).sum()))


# ---- 3. determinism, and what else lives on the context
def same(a, b):
    return all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


def test_same_bits_again_and_a_loaded_problem_survives(ctx, capi, golden):
    q, t = case("fpfh_range", 1500, 2000, 33)[:2]
    first = ctx.feature_match(q, t, mutual=True, want_d2=True)
    assert same(ctx.feature_match(q, t, mutual=True, want_d2=True), first)
    z = golden.npz("synth2k_clouds.npz")
    params = capi.icp_params(max_iterations=8)
    ctx.icp_load(z["before"], z["after"], params)
    ctx.icp_run(8)
    R0, t0, it0, err0, why0 = ctx.icp_result()
    ctx.icp_load(z["before"], z["after"], params)
    ctx.knn_search(None, z["after"], 8)
    ctx.feature_match(*case("mixed_sign", 65, 257, 64)[:2])
    assert same(ctx.feature_match(q, t, mutual=True, want_d2=True), first)
    ctx.icp_run(8)
    R1, t1, it1, err1, why1 = ctx.icp_result()
    assert it0 > 0 and (it1, why1) == (it0, why0)
    assert same((R1, t1), (R0, t0)) and np.float32(err1).tobytes() == np.float32(err0).tobytes()
    ms = ctx.feature_match_times()
    assert ms["total"] > 0 and ms["total"] >= ms["kernels"] >= 0


# ---- 4. refusals
def raw_call(ctx, capi, q, n, t, m, dim, mutual, null_idx=False):
    rows = max(min(n, 4096), 1)                       # (a call with more rows than that is one that is refused)
    idx, d2 = np.full(rows, -7, np.int32), np.full(rows, -7.5, np.float32)
    rc = capi.feature_match_raw(ctx._h, None if q is None else q.ctypes.data, n, None if t is None else t.ctypes.data, m, dim, mutual,
                                None if null_idx else idx.ctypes.data, d2.ctypes.data)
    return rc, capi.lib().mi_last_error().decode(), bool((idx == -7).all() and (d2 == -7.5).all())


def test_refusals_leave_the_outputs_untouched(ctx, capi):
    q, t = (np.array(a) for a in case("fpfh_range", 129, 257, 33)[:2])
    for args in ((None, 129, t, 257, 33, 0), (q, 129, None, 257, 33, 0), (q, 0, t, 257, 33, 0), (q, 129, t, 0, 33, 0), (q, -1, t, 257, 33, 1),
                 (q, 129, t, 257, 0, 0), (q, 129, t, 257, 65, 0), (q, 129, t, 257, 33, 2), (q, 129, t, 257, 33, -1)):
        rc, msg, untouched = raw_call(ctx, capi, *args)
        assert rc == capi.MI_ERR_INVALID_ARG and untouched and msg.startswith("mi_feature_match: "), (args[1:], msg)
    rc, msg, untouched = raw_call(ctx, capi, q, 129, t, 257, 33, 0, null_idx=True)
    assert rc == capi.MI_ERR_INVALID_ARG and untouched and msg.startswith("mi_feature_match: ")
    for args in ((q, (1 << 30) + 1, t, 257, 33, 0), (q, 129, t, (1 << 30) + 1, 33, 1)):       # refused before anything is read
        rc, msg, untouched = raw_call(ctx, capi, *args)
        assert rc == capi.MI_ERR_INVALID_ARG and untouched and msg.startswith("mi_feature_match: more than"), msg
    for value in (np.nan, np.inf, -np.inf, 1.1e15, -1.1e15):
        bq, bt = q.copy(), t.copy()
        bq[100, 32], bq[77, 0], bt[256, 5], bt[130, 1] = value, value, value, value
        rc, msg, untouched = raw_call(ctx, capi, q, 129, bt, 257, 33, 1)
        assert rc == capi.MI_ERR_INVALID_ARG and untouched and msg.startswith("mi_feature_match: ") and "target_feat row 130 " in msg, (value, msg)
        rc, msg, untouched = raw_call(ctx, capi, bq, 129, bt, 257, 33, 0)
        assert rc == capi.MI_ERR_INVALID_ARG and untouched and "query_feat row 77 " in msg, (value, msg)
    ok = q.copy()
    ok[3, 3] = -1e15                                  # the bound itself is admitted
    assert raw_call(ctx, capi, ok, 129, t, 257, 33, 1)[0] == capi.MI_OK
    with pytest.raises(capi.MiSlamError) as e:
        bt = t.copy()
        bt[5, 0] = np.nan
        ctx.feature_match(q, bt)
    assert "target_feat row 5 " in str(e.value)
