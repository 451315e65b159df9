"""CPU suite: the fp32 fmaf emulation and the restated contract of tests/match_reference.py, against hand-worked cases, exact rational
arithmetic one value at a time, a scalar loop, and the properties the contract of mi_feature_match relies on."""
import numpy as np

import match_reference as M

f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_fmaf_on_hand_worked_cases():
    # exact: 3 * 5 + 7
    assert M.fmaf(3, 5, 7) == f32(22)
    # one rounding, not two: (1 + 2^-23)^2 = 1 + 2^-22 + 2^-46; minus (1 + 2^-22) leaves the 2^-46 a separate multiply would have lost
    a = f32(1) + f32(2.0 ** -23)
    assert M.fmaf(a, a, -(f32(1) + f32(2.0 ** -22))) == f32(2.0 ** -46)
    assert f32(a * a) + -(f32(1) + f32(2.0 ** -22)) == f32(0)
    # a case ON an fp32 rounding tie once the sum has been rounded to float64: a * b = 2^36 - 2^-10 exactly, c = 2^60 + 2^37 (odd
    # significand, ulp 2^37).  The exact sum lies 2^-10 BELOW the midpoint c + 2^36, so fmaf gives c; the float64 sum IS the midpoint
    # (2^-10 is below float64's ulp of 2^8 there), and rounding that to fp32 goes to the even neighbour c + 2^37: the double rounding
    a, b = f32(2.0 ** 18) * (f32(1) + f32(2.0 ** -23)), f32(2.0 ** 18) * (f32(1) - f32(2.0 ** -23))
    c = f32(2.0 ** 60) + f32(2.0 ** 37)
    assert float(a) * float(b) == 2.0 ** 36 - 2.0 ** -10
    assert f32(float(a) * float(b) + float(c)) == f32(2.0 ** 60) + f32(2.0 ** 38)      # what the emulation must NOT give
    assert M.fmaf(a, b, c) == c and M.fmaf_scalar(a, b, c) == c
    # ... and the mirror image, 2^-10 above the midpoint below c: up to c again, where the float64 sum would go down to the even one
    assert M.fmaf(-a, b, c) == c and M.fmaf_scalar(-a, b, c) == c
    assert f32(-float(a) * float(b) + float(c)) == f32(2.0 ** 60)
    # a real tie stays a tie: 2^24 + 1 is the midpoint of 2^24 and 2^24 + 2 -> even
    assert M.fmaf(1, 1, f32(2.0 ** 24)) == f32(2.0 ** 24) and M.fmaf(1, 3, f32(2.0 ** 24)) == f32(2.0 ** 24 + 4)
    # zeros: fmaf(0, 0, c) = c, and +0 from -0
    assert bits(M.fmaf(0, 0, f32(-3.5))) == bits(f32(-3.5)) and bits(M.fmaf(0, 0, f32(-0.0))) == bits(f32(0.0))
    # fp32 subnormal results are rounded on the subnormal grid
    tiny = f32(2.0 ** -75)
    assert M.fmaf(tiny, tiny, 0) == f32(0) and M.fmaf(tiny, f32(2.0 ** -74), 0) == f32(2.0 ** -149)
    assert M.fmaf(f32(1.5) * tiny, f32(2.0 ** -74), 0) == f32(2.0 ** -148)             # 1.5 ulp: tie -> even


def test_fmaf_against_exact_rational_arithmetic():
    rng = np.random.default_rng(5)
    n = 3000
    scale = lambda: f32(2.0) ** rng.integers(-20, 21, n).astype(np.float32)
    a, b = (rng.normal(size=n).astype(np.float32) * scale() for _ in range(2))
    c = -(a.astype(np.float64) * b.astype(np.float64)).astype(np.float32)              # heavy cancellation in the first third
    c[n // 3:] = (rng.normal(size=n - n // 3).astype(np.float32) * scale()[n // 3:])
    # rows built next to fp32 midpoints: a * b = +-(2^-24 - 2^-70) under c in [1, 1 + 2^-21]: the float64 sum is the midpoint itself
    a[-200:] = f32(2.0 ** -12) * (f32(1) + f32(2.0 ** -23))
    b[-200:] = f32(2.0 ** -12) * (f32(1) - f32(2.0 ** -23)) * rng.choice([-1.0, 1.0], 200).astype(np.float32)
    c[-200:] = f32(1) + f32(2.0 ** -23) * rng.integers(0, 4, 200).astype(np.float32)
    got = M.fmaf(a, b, c)
    want = np.array([M.fmaf_scalar(x, y, z) for x, y, z in zip(a, b, c)], np.float32)
    assert np.array_equal(bits(got), bits(want))
    naive = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
    assert (bits(naive) != bits(want)).any()          # the catalogue does hold cases that a double rounding gets wrong


def test_chain_against_a_scalar_loop():
    rng = np.random.default_rng(6)
    q, t = rng.uniform(0, 200, (5, 33)).astype(np.float32), rng.uniform(-200, 200, (7, 33)).astype(np.float32)
    dot = M.chain(q, t)
    tt = M.norms(t)
    for i in range(5):
        for j in range(7):
            c = f32(0)
            for b in range(33):
                c = M.fmaf_scalar(q[i, b], t[j, b], c)
            assert bits(c) == bits(dot[i, j])
    for j in range(7):
        c = f32(0)
        for b in range(33):
            c = M.fmaf_scalar(t[j, b], t[j, b], c)
        assert bits(c) == bits(tt[j])
    h, g = M.keys(q, t)
    assert bits(h[2, 3]) == bits(M.fmaf_scalar(-2.0, dot[2, 3], tt[3])) and bits(g[3, 2]) == bits(M.fmaf_scalar(-2.0, dot[2, 3], M.norms(q)[2]))


def test_chain_is_symmetric_and_zero_padding_is_neutral():
    rng = np.random.default_rng(7)
    q, t = rng.normal(size=(40, 33)).astype(np.float32), rng.normal(size=(50, 33)).astype(np.float32)
    q[3], t[4] = 0, 0                                 # zero rows: +0 sums
    q[5, :30], t[5, :30] = 0, 0
    assert np.array_equal(bits(M.chain(q, t)), bits(M.chain(t, q).T))
    pad = lambda x, k: np.concatenate([x, np.zeros((len(x), k), np.float32)], axis=1)
    for k in (1, 31):
        assert np.array_equal(bits(M.chain(pad(q, k), pad(t, k))), bits(M.chain(q, t)))
        assert np.array_equal(bits(M.norms(pad(t, k))), bits(M.norms(t)))
    # a product that underflows to -0 leaves the chain at -0, which the padding turns into +0: the same key, the same comparison
    tiny = np.array([[2.0 ** -80, 0.0]], np.float32)
    dot = M.chain(tiny, -tiny)
    assert bits(dot)[0, 0] == 0x80000000 and bits(M.chain(pad(tiny, 2), pad(-tiny, 2)))[0, 0] == 0
    assert bits(M.fmaf(-2.0, dot, f32(0)))[0, 0] == 0 and bits(M.fmaf(-2.0, f32(0), f32(0))) == 0


def test_key_orders_as_the_distance_and_low_index_wins():
    rng = np.random.default_rng(8)
    q, t = rng.uniform(0, 200, (60, 33)).astype(np.float32), rng.uniform(0, 200, (90, 33)).astype(np.float32)
    t[70], t[20] = t[11], t[11]                       # exact duplicates: the lowest index is the answer
    q[0] = t[70]
    idx, d2, fwd, rev = M.match(q, t)
    assert idx[0] == 11 and d2[0] == 0
    exact = ((q.astype(np.float64)[:, None, :] - t.astype(np.float64)[None, :, :]) ** 2).sum(axis=2)
    # the key's error is a few fp32 roundings of |q|^2 + |t|^2 ~ 1e6: the chosen target is within that of the float64 minimum
    assert (exact[np.arange(60), idx] - exact.min(axis=1) <= 64 * 2.0 ** -23 * 4e6).all()
    kept, want = M.d2_float64(q, t, idx)
    assert kept.all() and (np.abs(d2 - want) <= 2.0 ** -23 * want).all()
    midx, md2, _, _ = M.match(q, t, mutual=True)
    assert ((midx == idx) | (midx == -1)).all() and (midx >= 0).any() and (midx < 0).any()
    assert np.isinf(md2[midx < 0]).all() and np.array_equal(md2[midx >= 0], d2[midx >= 0])
    assert len(set(midx[midx >= 0])) == int((midx >= 0).sum())      # a mutual match is one to one
    for i in np.flatnonzero(midx >= 0):
        assert rev[midx[i]] == i
