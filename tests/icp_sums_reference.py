"""A float64 reference of the sums of one point-to-point ICP iteration -- the 16 moments and 2 error sums of csrc/icp_rows.hpp -- of the
solve that reads them and of the composition behind it.  numpy only.  Shared by tests/test_icp_sums_reference.py (CPU: against the oracle on
the bunny fixture, and the mutation checks that give the bounds their teeth) and tests/test_gpu_icp_sums.py (every producer and reducer of
the sums on the device).

  transform(b, R, t)                ((R0 x + R3 y) + R6 z) + t0 in float32, one rounding per operation: the fused search's and K4/K5's own
                                    arithmetic (plane_reference.move_f32 is that very expression: reused)
  moments(b_cur, a_matched, use)    (sums [16], sums of the terms' magnitudes [16]) in the layout of kernels.h: count, sum b (3), sum a (3),
                                    sum a_r b_c (9, row-major in r).  b = the moving point where the search saw it, a = its match
  error_sums(a_matched, b_new, kept)   ([sum e, kept pairs], magnitudes): e = (dx dx + dy dy) + dz dz in float32 as the kernels write it (e0
                                    has this non-FMA form in both dist modes), the float32 values summed in extended precision
  additions(n, route), bounds(n, route, magnitudes)   k and k 2^-53 sum|term|, below
  solve(mom), compose(R, t, Ri, ti, compose_mode), solve_bars(...)   solve_from_moments / apply_solve (icp_solve.hpp) in float64

A term of a moment is 1, a float32 value or a product of two (24 + 24 bits: exact in float64); the sums are taken in np.longdouble
(pairwise) and kept there: the reference's own error is below 2^-60 of the sum of the magnitudes.

The bound of a sum is k 2^-53 sum|term|, k = the longest chain of fp64 additions a term goes through on its way into the state, counted
from the code (nothing here is measured):
  in a row (row_store_pair_moments / row_store_error, icp_rows.hpp): a term enters one of four chained matrix-pipe products D = A B + C, each
    a contraction over 4 -- whatever the unit's order inside, C and four products are added in a chain of at most 4 -- so a term of the
    first product has gone through at most 4 x 4 additions behind the fourth; then the two row rotations: ROW_CHAIN = 18;
  sum_row_slice (icp_rows_reduce_kernel, icp_rows_reduce_solve_kernel): a strip adds its rows of the slice, ceil(slice / 56) of them (the
    first to 0.0), then the 56 strips are added in order: + ceil(slice / 56) + 55, slice = ceil(rows / reduced rows);
  icp_reduce_solve_kernel (rows <= ICP_FUSED_SOLVE_MAX_ROWS): 0.0 + row, the 32 rows of a slice chained, + 0.0: + 1 + 31 + 1;
  reduce_rows_wave: the halving butterfly over the 64 lanes, 6 levels for every column: + 6;
  a distributed context all-reduces the 64 reduced rows (those past its own count are zeros) over its ranks: + world - 1 (none at world 1).
The two counts are sums of ones: integers below 2^53, exact in any order -- bound 0, as for every sum whose terms are all zero."""
import numpy as np

import plane_reference as P
from kabsch_catalogue import EPS, kabsch64, posedness

U64 = 2.0 ** -53
ROW_POINTS = 64                    # ICP_ROW_POINTS
REDUCED_ROWS = 64                  # ICP_REDUCED_ROWS
STRIPS = 1024 // 18                # ROWS_REDUCE_STRIPS
FUSED_SOLVE_MAX_ROWS = 2048        # ICP_FUSED_SOLVE_MAX_ROWS
ROW_CHAIN = 4 * 4 + 2
BUTTERFLY = 6
ROUTES = ("one_workgroup", "ticket", "two_launch", "world1")


def transform(b, R, t):
    """R [3, 3] indexed [row, col] (the state's column-major R9[3 c + r]), t [3]; float32 in, float32 out."""
    return P.move_f32(np.asarray(R, np.float32), np.asarray(t, np.float32), b)


def _sum(v):
    return np.sum(np.asarray(v, np.longdouble))


def pair_terms(b, a):
    """[n, 16] float64: every pair's exact terms of the 16 moments."""
    b, a = np.asarray(b, np.float32).astype(np.float64).reshape(-1, 3), np.asarray(a, np.float32).astype(np.float64).reshape(-1, 3)
    cross = (a[:, :, None] * b[:, None, :]).reshape(-1, 9)           # a_r b_c, row-major in r
    return np.concatenate([np.ones((len(b), 1)), b, a, cross], axis=1)


def moments(b_cur, a_matched, use):
    use = np.asarray(use, bool)
    T = pair_terms(b_cur, a_matched)[use]
    mom, mag = np.zeros(16, np.longdouble), np.zeros(16, np.longdouble)
    for c in range(16):
        mom[c], mag[c] = _sum(T[:, c]), _sum(np.abs(T[:, c]))
    return mom, mag


def pair_errors(a_matched, b_new):
    """float32 [n]: (dx dx + dy dy) + dz dz with d = a - b', every operation rounded to float32."""
    a, b = np.asarray(a_matched, np.float32).reshape(-1, 3), np.asarray(b_new, np.float32).reshape(-1, 3)
    d = a - b
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def error_sums(a_matched, b_new, kept):
    kept = np.asarray(kept, bool)
    e = pair_errors(a_matched, b_new)[kept]
    assert e.dtype == np.float32
    err = np.array([_sum(e), np.longdouble(int(kept.sum()))], np.longdouble)
    return err, err.copy()                                          # (e >= 0: the magnitudes are the sums)


def row_count(n):
    return (n + ROW_POINTS - 1) // ROW_POINTS


def reduced_count(nrows):                                           # icp_reduced_count (icp_kernels.hip)
    return max(1, min(REDUCED_ROWS, (nrows + 31) // 32))


def additions(n, route, world=1):
    """k of the module docstring for a moving cloud of n points on a reducer route."""
    assert route in ROUTES
    nrows = row_count(n)
    per = -(-nrows // reduced_count(nrows))
    if route == "one_workgroup":
        assert nrows <= FUSED_SOLVE_MAX_ROWS and per <= FUSED_SOLVE_MAX_ROWS // REDUCED_ROWS
        k = ROW_CHAIN + 1 + (FUSED_SOLVE_MAX_ROWS // REDUCED_ROWS - 1) + 1
    else:
        k = ROW_CHAIN + -(-per // STRIPS) + (STRIPS - 1)
    k += BUTTERFLY
    if route == "world1":
        k += world - 1
    return k


def bounds(n, route, magnitudes, world=1):
    """|device - reference| allowed per sum: k 2^-53 sum|term|; 0 for the counts."""
    out = additions(n, route, world) * U64 * np.asarray(magnitudes, np.float64)
    if len(out) == 16:
        out[0] = 0.0
    else:
        out[1] = 0.0
    return out


def routes_at(n):
    """The reducer routes a cloud of n moving points can take (icp_enqueue_iteration): one workgroup up to ICP_FUSED_SOLVE_MAX_ROWS rows,
    the ticket form beyond (and below, under MISLAM_ICP_FUSED_SOLVE=0), the two launches under both switches, the distributed form."""
    return (("one_workgroup",) if row_count(n) <= FUSED_SOLVE_MAX_ROWS else ()) + ("ticket", "two_launch", "world1")


# ---- the solve and the composition (icp_solve.hpp solve_from_moments, apply_solve) in float64 ----
def solve(mom):
    """-> dict(R [3, 3] indexed [row, col], t, ca, cb, S, g, cond, well): H = sum a b^T - n ca cb^T, R = U diag(1, 1, det(U V^T)) V^T -- the
    determinant rule of svd3.hpp, as kabsch_catalogue.kabsch64 states it -- and t = ca - R cb."""
    mom = np.asarray(mom, np.float64)
    n = mom[0]
    cb, ca = mom[1:4] / n, mom[4:7] / n
    H = mom[7:16].reshape(3, 3) - n * np.outer(ca, cb)
    R, S, d, g = kabsch64(H[None])
    cond, well, _ = posedness(S, g)
    return dict(R=R[0], t=ca - R[0] @ cb, ca=ca, cb=cb, S=S[0], g=float(g[0]), cond=float(cond[0]), well=bool(well[0]), H=H)


def compose(R, t, Ri, ti, compose_mode):
    """compose_mode 0 (MI_COMPOSE_CPU_ADDITIVE): R <- Ri R, t <- ti + t; 1 (MI_COMPOSE_EXACT): R <- Ri R, t <- Ri t + ti."""
    R, t, Ri, ti = (np.asarray(x, np.float64) for x in (R, t, Ri, ti))
    return Ri @ R, (ti + t if compose_mode == 0 else Ri @ t + ti)


def solve_bars(sol, t_prev, compose_mode):
    """(bar of |R_k - reference| per entry, bar of |t_k - reference| per entry) for a well-posed solve, from the fp32 operations between the
    moments and the state:
      Ri: tests/test_gpu_kabsch3.py holds the solve of an fp32 H within 32 (eps sigma_1 / g + eps) of the float64 Kabsch; here H's entries
        are rounded to fp32 first (eps / 2 each, |dH| <= 1.5 eps sigma_1, R moves by |dH| / g): 34 (eps sigma_1 / g + eps);
      ti = fca - ((Ri0 fcb0 + Ri3 fcb1) + Ri6 fcb2): that test's own translation bar, 3 max|cb| |dRi| + 8 eps (max|ca| + 3 max|cb|);
      R_k = Ri R in fp32: |dRi R| <= sqrt(3) |dRi| (a column of R has 1-norm <= sqrt 3), three products and two additions on terms whose
        magnitudes sum to <= 1: + 2 eps;
      t_k = ti + t: + eps (|ti| + |t|) for the addition; or ((Ri0 t0 + Ri3 t1) + Ri6 t2) + ti: 3 max|t| |dRi| + 4 eps (3 max|t| + max|ti|)."""
    assert sol["well"]
    bar_ri = 34.0 * (sol["cond"] + EPS)
    ca, cb, tp, ti = (float(np.abs(x).max()) for x in (sol["ca"], sol["cb"], t_prev, sol["t"]))
    bar_ti = 3.0 * cb * bar_ri + 8.0 * EPS * (ca + 3.0 * cb)
    bar_r = np.sqrt(3.0) * bar_ri + 2.0 * EPS
    if compose_mode == 0:
        bar_t = bar_ti + EPS * (ti + tp)
    else:
        bar_t = bar_ti + 3.0 * tp * bar_ri + 4.0 * EPS * (3.0 * tp + ti)
    return bar_r, bar_t


# ---- the inputs of the two test modules ----
N_THRESHOLD = ROW_POINTS * FUSED_SOLVE_MAX_ROWS + ROW_POINTS          # one row past the one-workgroup form (tests/test_gpu_icp_ticket_solve.py)
N_RAGGED = ROW_POINTS * (FUSED_SOLVE_MAX_ROWS + 140) - 17             # rows no multiple of the summing workgroups, a partly filled last row
# partly filled quads (1, 2, 3, 5), partly filled rows (63, 65, 255, 4097), one row past a wave of rows (4097), the reducer edges
SIZES = (1, 2, 3, 5, 63, 64, 65, 255, 4097, ROW_POINTS * FUSED_SOLVE_MAX_ROWS, N_THRESHOLD, N_RAGGED)
M_FIXED = 3000                    # the fixed cloud: large enough for a search index, small enough for an every-pair reference search
LO, HI = 4.0, 12.0                 # every coordinate stays away from zero: one fp32 ulp of any of them is visible in the sums (mutation checks)


def rotation(angle=0.2):
    axis = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def clouds(n, seed=None, m=M_FIXED):
    """(moving [n, 3], fixed [m, 3]) float32: the moving cloud uniform in the cube [LO, HI]^3; the fixed cloud m points of the same
    distribution turned by 0.2 rad about the cube's centre, shifted and jittered -- no symmetry, no repeated point, no coordinate near zero."""
    rng = np.random.default_rng(1000 + n if seed is None else seed)
    before = rng.uniform(LO, HI, (n, 3))
    centre = 0.5 * (LO + HI)
    after = (rng.uniform(LO, HI, (m, 3)) - centre) @ rotation().T + centre + (0.3, -0.2, 0.25) + rng.normal(scale=0.02, size=(m, 3))
    return before.astype(np.float32), after.astype(np.float32)


def median_filter(d2):
    """max_distance_squared a hair above the median d2: about half the pairs drop out, in no regular pattern, and one point keeps its pair."""
    return float(np.nextafter(np.float32(np.median(np.asarray(d2, np.float32))), np.float32(np.inf)))


def nearest(cur, after):
    """Every-pair nearest neighbour in float64 (a CPU stand-in for the device search where no device is at hand): (idx, d2 float32)."""
    cur, after = np.asarray(cur, np.float64), np.asarray(after, np.float64)
    idx, d2 = np.empty(len(cur), np.int64), np.empty(len(cur))
    a2 = (after * after).sum(axis=1)
    for lo in range(0, len(cur), 8192):
        c = cur[lo:lo + 8192]
        d = (c * c).sum(axis=1)[:, None] + a2[None, :] - 2.0 * (c @ after.T)
        idx[lo:lo + 8192] = d.argmin(axis=1)
        d2[lo:lo + 8192] = d.min(axis=1)
    return idx, np.maximum(d2, 0.0).astype(np.float32)
