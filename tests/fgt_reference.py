"""A seeded catalogue of Fast-Gauss-Transform E-step problems (ComputePMatrixWithFGT, cpdutils.cpp:19-77) and two float64 references,
with per-element error bounds.  Shared by tests/test_fgt_reference.py (CPU: the bound model against the oracle, the plan coverage, the
mutation check, the overflow case) and tests/test_gpu_fgt_estep.py (every case through mi_cpd_estep_fgt on several contexts).  Generated in
code: the same seed gives the same float32 clouds on every machine.

The E-step runs two transforms v(q) = sum_k [ |dy|^2 <= e ] e^{-|dy|^2} sum_a B_ka dy^a, B_ka = C_a sum_{i in k} w_i e^{-|dx_i|^2} dx_i^a,
dx = (s_i - c_k) inv, dy = (q - c_k) inv, inv = 1 / sqrt(2 sigma^2) (float32): the moving cloud with unit weights queried at the fixed cloud
(Kt1), then the fixed cloud weighted by 1/den and x/den queried at the moving cloud (P1, PX); den = Kt1 + ndi.

References (both from the same float32 inputs, the same K-centre labels and means -- oracle.fgt_kcenter, bit for bit the device's):
  A "FGT in float64": dx, dy and their squared lengths are formed in float32 exactly as the kernels form them ((p - c) * inv, then
    (x*x + y*y) + z*z; the library is built with -ffp-contract=off, so numpy's float32 arithmetic gives the same bits), so the reached set
    |dy|^2 > e is decided on the kernels' bits.  C_a is the reference's float32 ComputeC_k table (oracle.fgt_ck); the monomial exponents
    come from the recursion of fgt.cpp written out here, not from the library's tables.  Everything else -- exp, the monomials, every sum,
    1/den, Pt1, the weights and L -- is float64.  A NaN cell mean (an empty cell) is reached by every query and propagates (fgt.cpp:120).
  B "the series in closed form": the same float32 offsets and reached set; each pair is w exp(-|dx|^2 - |dy|^2 + 2 dx.dy) in float64 (the
    Gaussian the truncated series approximates), plus the Taylor remainder of every pair in reach as an allowance,
    |w| e^{-|dx|^2-|dy|^2} (2|dx||dy|)^p / p! e^{2|dx||dy|}, and the float32 exponents' conditioning 3u (|dx|^2 + |dy|^2) per term.
    Computed where at most B_MAX_PAIRS pairs are in reach.

Bounds, per element, normalised by the sum of the absolute values of the element's terms (never by an array maximum), u = 2^-24:
  T_q = sum_{k in reach} e_qk sum_a |B|_ka |dy^a|,  |B|_ka = C_a sum_{i in k} |w_i| e_i |dx_i^a|
  v_q   u (4 + sqrt(depth)) T_q  (depth: the model chain -- a group's members, the G group adds, the Z partial adds, x C_a -- the p + 2
        products of a term, the 2(p - 1) Horner steps, the K/S cells of a split and the S partial adds; 4: expf on both sides)
  P1/PX + the error carried in through the weights: a third coefficient set with weights |w_x| eps_x, eps_x = bound(Kt1_x)/den_x + u
  Pt1   (ndi/den) bound(Kt1)/den + 2u (1 + ndi/den)
  L     sum_x (bound(Kt1_x)/den_x + 4u + u |log den_x|) + u (|L| + 2 |1.5 n log sigma^2|)
plus FLT_MIN per term the kernels may flush.  The bar on |kernel - reference| / bound is BAR, fixed before any GPU measurement."""
import math

import numpy as np

U = 2.0 ** -24
FLT_MIN = float(np.finfo(np.float32).tiny)
BAR = 16.0
FGT_TILE, FGT_MODEL_GROUPS, FGT_MODEL_MAX_SPLITS, FGT_MAX_ORDER = 128, 4, 16, 16          # cpd_fgt.hip / cpd_fgt.h
LISTS_MAX_POINTS, LISTS_MAX_READS = 32768, 4 << 20
COOP_MIN_POINTS, COOP_MAX_POINTS, GRID_SWEEP_MIN_POINTS = 16 * 1024, 64 * 1024 * 16, 65536
B_MAX_PAIRS = 60_000_000
WEIGHTS = (1e-6, 0.3, 1.0 - 1e-6)
CONTEXTS = {"default": None, "splits0": ("MISLAM_FGT_MODEL_SPLITS", "0"), "lists0": ("MISLAM_FGT_LISTS_IN_MODEL", "0"),
            "coop0": ("MISLAM_FGT_COOP_SWEEP", "0"), "coop2": ("MISLAM_FGT_COOP_SWEEP", "2")}
f32 = np.float32


# ---- the plan (cpd_plan.hpp, cpd_fgt_api.hip cpd_estep_fgt_enqueue, cpd_fgt.hip; tests/test_cpd_plan.py holds the first to these) ----
def cluster_count(m, n, sigma2, sigma2_init):
    """fgt_cluster_count: (int) std::round(min(n, m, 50 + s2i / s2)) in float."""
    k = min(f32(n), f32(m), f32(50.0) + f32(sigma2_init) / f32(sigma2))
    return int(math.floor(float(k) + 0.5))


def hsigma_inv(sigma2):
    h = np.sqrt(f32(2.0) * f32(sigma2))                       # sqrtf: correctly rounded
    return f32(h), f32(1.0) / f32(h)


def ndi(sigma2, weight, m, n):
    """fgt_ndi: pow and the numerator in double, (1 - weight) * n a float product."""
    den = f32(f32(1.0) - f32(weight)) * f32(n)
    return float(f32((math.pow(2 * math.pi * float(f32(sigma2)), 1.5) * float(f32(weight)) * m) / float(den)))


def pd_of(p):
    return p * (p + 1) * (p + 2) // 6


def lists_rule(n, K):
    return n <= LISTS_MAX_POINTS and K * n <= LISTS_MAX_READS


def model_splits(n, K, pd):
    ny = (pd + FGT_TILE - 1) // FGT_TILE
    z = (n // max(K, 1)) // (FGT_TILE * FGT_MODEL_GROUPS)
    z = min(z, 1024 // max(K * ny, 1), FGT_MODEL_MAX_SPLITS)
    return max(1, z)


def predict_splits(nq, K):
    waves = (nq + 63) // 64
    return max(1, min((4096 + waves - 1) // waves, 16, K))


def side_plan(n_side, K, pd, context="default"):
    """(Z, path) of one side's model build on a context: the `splits` lambda of cpd_estep_fgt_enqueue."""
    lists = context != "lists0"
    in_model = lists and lists_rule(n_side, K)
    if context == "splits0" or in_model:
        z = 1
    else:
        z = model_splits(n_side, K, pd)
    return z, ("lists" if in_model else "sort")


def sweep(n_side, K, context="default"):
    """Which K-centre sweep a first clustering of n_side points runs (fgt_cluster)."""
    coop = {"coop0": 0, "coop2": 2}.get(context, 1)
    if COOP_MIN_POINTS < n_side <= COOP_MAX_POINTS and (coop == 2 or (coop == 1 and K >= 16)):
        return "coop"
    if n_side > GRID_SWEEP_MIN_POINTS:
        return "grid"
    return "one_wg"


def plan(case, context="default"):
    m, n, p = case.m, case.n, case.p
    K = cluster_count(m, n, case.sigma2, case.sigma2_init)
    pd = pd_of(p)
    zy, py = side_plan(m, K, pd, context)
    za, pa = side_plan(n, K, pd, context)
    return dict(K=K, pd=pd, yblocks=(pd + FGT_TILE - 1) // FGT_TILE, Zy=zy, Za=za, path_y=py, path_a=pa,
                Sa=predict_splits(n, K), Sy=predict_splits(m, K), horner="p8" if p == 8 else "generic",
                sweep_y=sweep(m, K, context), sweep_a=sweep(n, K, context))


# ---- the catalogue ----
class Case:
    def __init__(self, name, cls, y, x, sigma2, weight, p, e=10.0, sigma2_init=None, big=False):
        self.name, self.cls = name, cls
        self.y, self.x = np.ascontiguousarray(y, np.float32), np.ascontiguousarray(x, np.float32)
        self.sigma2 = float(f32(sigma2))
        self.sigma2_init = float(f32(sigma2_init if sigma2_init is not None else sigma2))
        self.weight = float(f32(weight))
        self.p, self.e = int(p), float(f32(e))
        self.big = big

    @property
    def m(self):
        return len(self.y)

    @property
    def n(self):
        return len(self.x)

    def __repr__(self):
        return "%s(%d x %d, sigma2 %g, w %g, p %d, e %g)" % (self.name, self.m, self.n, self.sigma2, self.weight, self.p, self.e)


def _uniform(rng, k, half=5.0):
    return rng.uniform(-half, half, (k, 3))


def _near(rng, base, k, scale=0.3):
    return base[rng.integers(0, len(base), k)] + rng.normal(scale=scale, size=(k, 3))


def _lattice(k, spacing=1.0):
    side = int(math.ceil(k ** (1.0 / 3.0)))
    g = np.arange(side, dtype=np.float64) * spacing
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)[:k]


def far_members(rng, half, sigma2, p, kcenter):
    """The overflow case: 1 000 fixed points uniform in [-half, half]^3 in K = 2 cells (m = 2), the two moving points next to the two cell
    means, so that every query reaches a cell whose members sit hundreds of sigmas from its mean: d^(p-1) overflows float32 while
    exp(-|d|^2) is exactly 0."""
    x = f32(_uniform(rng, 1000, half))
    xc, _ = kcenter(x, 2)
    return xc.astype(np.float64) + np.array([0.05, -0.03, 0.02]), x


def catalogue(seed=20261017, with_big=True, kcenter=None):
    """Every case of the catalogue.  kcenter (oracle.fgt_kcenter) places the overflow cases' queries; without it they are left out."""
    rng = np.random.default_rng(seed)
    cases = []
    wi = [0]

    def add(name, cls, y, x, sigma2, p, **kw):
        cases.append(Case(name, cls, y, x, sigma2, WEIGHTS[wi[0] % 3], p, **kw))
        wi[0] += 1

    # uniform clouds: the P == 8 Horner, ragged query counts around 64 (the last wave holds 63 / 64 / 1 queries)
    y = _uniform(rng, 300); add("uniform_300x500_p8", "uniform", y, _near(rng, y, 500, 1.0), 1.0, 8, sigma2_init=10.0)
    y = _uniform(rng, 63); add("uniform_63x1000_p5", "uniform", y, _near(rng, y, 1000, 0.5), 2.0, 5)
    y = _uniform(rng, 64); add("uniform_64x4097_p3", "uniform", y, _near(rng, y, 4097, 0.5), 0.5, 3, sigma2_init=50.0)
    y = _uniform(rng, 65); add("uniform_65x129_p2", "uniform", y, _near(rng, y, 129, 0.5), 0.3, 2)
    y = _uniform(rng, 200); add("uniform_200x300_p1", "uniform", y, _near(rng, y, 300, 0.5), 0.7, 1, e=1.0)
    # clustered blobs at order 11 (pd = 286 > FGT_TILE: three y-blocks) and 16 (FGT_MAX_ORDER)
    centres = _uniform(rng, 12)
    add("blobs_1500x2000_p11", "blobs", _near(rng, centres, 1500), _near(rng, centres, 2000), 0.5, 11)
    add("blobs_700x900_p16", "blobs", _near(rng, centres, 700), _near(rng, centres, 900), 0.8, 16, e=100.0)
    # exactly planar (dz = 0: the monomials' 0^0 = 1 and 0^c = 0)
    y = _uniform(rng, 400); y[:, 2] = 0
    x = _near(rng, y, 600); x[:, 2] = 0
    add("planar_400x600_p5", "planar", y, x, 0.3, 5)
    # integer lattice: K-centre ties, exact distance ties
    add("lattice_343x512_p8", "lattice", _lattice(343), _lattice(512) - 0.5, 0.6, 8)
    # duplicates: more cells than distinct points -> empty cells, NaN means; moving side (everything NaN) / fixed side (P1, PX NaN)
    few = _uniform(rng, 6)
    add("duplicate_moving_30x40_p5", "duplicate", np.repeat(few, 5, axis=0), _near(rng, few, 40), 1.0, 5, sigma2_init=1e4)
    few = _uniform(rng, 10)
    add("duplicate_fixed_200x80_p5", "duplicate", _near(rng, few, 200), np.repeat(few, 8, axis=0), 1.0, 5, sigma2_init=1e4)
    # offset by 1e3; 5 % far outliers
    y = _uniform(rng, 800) + 1e3; add("offset_800x1200_p8", "offset", y, _near(rng, y, 1200), 0.5, 8)
    y = _uniform(rng, 1000); x = _near(rng, y, 1000)
    y[rng.permutation(1000)[:50]] += 1e3; x[rng.permutation(1000)[:50]] -= 1e3
    add("outliers_1000x1000_p8", "outliers", y, x, 0.5, 8)
    # sigma^2 over four decades on one pair of clouds; e = 1 / 100
    y = _uniform(rng, 1000); x = _near(rng, y, 1100, 0.5)
    for s2, p, e in ((0.01, 8, 10.0), (0.1, 5, 100.0), (1.0, 8, 1.0), (100.0, 3, 10.0)):
        add("sigma2_%g_1000x1100_p%d_e%g" % (s2, p, e), "sigma2", y, x, s2, p, e=e)
    # the full mode's clamp (sigma^2 = 0.05) on a cloud with coordinates in the hundreds
    y = _uniform(rng, 1000, 300.0); add("clamp_1000x1500_p8", "clamp", y, _near(rng, y, 1500, 0.2), 0.05, 8, sigma2_init=5e4)
    # K = min(m, n): one point per cell on both sides
    y = _uniform(rng, 256); add("one_per_cell_256x256_p5", "one_per_cell", y, _near(rng, y, 256, 0.1), 0.2, 5, sigma2_init=1e3)
    # isolated sources, one per cell, queried 7.7 sigma away (|dy|^2 = 60, near the far field e = 100) at a sigma^2 whose float32 inv is
    # 1.47 u off 1 / sqrt(2 sigma^2): each value is one Gaussian, and the exact h moves it by 2 x 1.47 u x 60
    s2 = 1.9055
    y = _lattice(64, 40.0)
    dirs = rng.normal(size=(64, 3))
    x = y + dirs / np.linalg.norm(dirs, axis=1, keepdims=True) * math.sqrt(60.0 * 2.0 * s2)
    add("isolated_64x64_p1_e100", "isolated", y, x, s2, 1, e=100.0, sigma2_init=1e3)
    # big cells: m = 2 (K = 2) against 30 000 points (the lists path; split 16 ways on a lists0 context) and 40 000 (the sort path, Z = 16)
    x = f32(_uniform(rng, 30000, 2.0)); add("bigcell_2x30000_p11", "bigcell", x[[3, 4]] * 0.5, x, 1.0, 11)
    x = f32(_uniform(rng, 40000, 2.0)); add("bigcell_2x40000_p8", "bigcell", x[[5, 6]] * 0.5, x, 1.0, 8)
    # the overflow case: members hundreds of sigmas from their cell mean (p = 16 at sigma^2 = 1, p = 12 at the full-mode clamp)
    if kcenter is not None:
        y, x = far_members(rng, 1000.0, 1.0, 16, kcenter); add("far_members_2x1000_p16", "far_members", y, x, 1.0, 16)
        y, x = far_members(rng, 2000.0, 0.05, 12, kcenter); add("far_members_2x1000_p12", "far_members", y, x, 0.05, 12)
    # Z > 1 at 51 cells, the cooperative / grid-wide sweeps (more than 65 536 points), S = 1 on the fixed side (nq > 262 080)
    y = _uniform(rng, 150000, 4.0); add("split_150000x120000_p8", "split", y, _near(rng, y, 120000, 0.2), 2.0, 8)
    y = _uniform(rng, 70000, 6.0); add("sweep_70000x300000_p5", "split", y, _near(rng, y, 300000, 0.2), 1.5, 5)
    if with_big:
        y = _uniform(rng, 1000000, 5.0); add("big_1000000x1000000_p3", "split", y, _near(rng, y, 1000000, 0.2), 3.0, 3, big=True)
    return cases


def coverage(cases):
    """What the catalogue reaches of the plan, per requirement -> the cases that reach it (default context unless named)."""
    cov = {}

    def hit(key, case):
        cov.setdefault(key, []).append(case.name)
    for c in cases:
        pl = plan(c)
        K = pl["K"]
        hit("order=%d" % c.p, c)
        hit("e=%g" % c.e, c)
        hit("horner_" + pl["horner"], c)
        if K == 2:
            hit("K=2", c)
        if K == min(c.m, c.n):
            hit("K=min(m,n)", c)
        if pl["yblocks"] > 1:
            hit("pd>FGT_TILE", c)
        for nq in (c.m, c.n):
            if nq % 64 in (0, 1, 63):
                hit("nq%%64=%d" % (nq % 64), c)
        for s in (pl["Sa"], pl["Sy"]):
            if s in (1, 16):
                hit("S=%d" % s, c)
        if "lists" in (pl["path_y"], pl["path_a"]):
            hit("lists_path", c)
        if "sort" in (pl["path_y"], pl["path_a"]):
            hit("sort_path", c)
        if max(pl["Zy"], pl["Za"]) > 1:
            hit("Z>1", c)
        pl0 = plan(c, "lists0")
        if max(pl0["Zy"], pl0["Za"]) > 1 and max(pl["Zy"], pl["Za"]) == 1:
            hit("Z>1_only_without_lists", c)
        if "coop" in (pl["sweep_y"], pl["sweep_a"]):
            hit("coop_sweep", c)
        if "grid" in (plan(c, "coop0")["sweep_y"], plan(c, "coop0")["sweep_a"]):
            hit("grid_sweep", c)
        hit("weight=%g" % c.weight, c)
        hit("class=" + c.cls, c)
        if c.sigma2 == float(f32(0.05)) and np.abs(c.x).max() >= 100:
            hit("clamp_large_coords", c)
    return cov


REQUIRED_COVERAGE = ["order=%d" % p for p in (1, 2, 3, 5, 8, 11, 16)] + ["e=1", "e=10", "e=100", "horner_p8", "horner_generic", "K=2",
                     "K=min(m,n)", "pd>FGT_TILE", "nq%64=0", "nq%64=1", "nq%64=63", "S=1", "S=16", "lists_path", "sort_path", "Z>1",
                     "Z>1_only_without_lists", "coop_sweep", "grid_sweep", "clamp_large_coords"] + \
                    ["class=" + k for k in ("uniform", "blobs", "planar", "lattice", "duplicate", "offset", "outliers", "sigma2",
                                            "one_per_cell", "isolated", "bigcell", "far_members", "split")]


# ---- the monomials (fgt.cpp's graded recursion, written out) ----
def exponents(p):
    """(a, b, c) of monomial t in the reference's order: prods[0] = 1; degree by degree, coordinate i multiplied onto the previous degree's
    monomials from heads[i] on (fgt.cpp:124-137, the oracle's `monomials`)."""
    ex = [(0, 0, 0)]
    heads = [0, 0, 0]
    t = tail = 1
    for _ in range(1, p):
        for i in range(3):
            head, heads[i] = heads[i], t
            for j in range(head, tail):
                e = list(ex[j])
                e[i] += 1
                ex.append(tuple(e))
                t += 1
        tail = t
    return np.array(ex, np.int64).reshape(-1, 3)


def _mono(d, ex):
    """d^a for every row of d (float64) and every exponent row of ex: the powers of each coordinate, then their products."""
    p = int(ex.max()) + 1 if len(ex) else 1
    pw = np.ones((3, len(d), p))
    for r in range(1, p):
        pw[:, :, r] = pw[:, :, r - 1] * d.T
    return pw[0][:, ex[:, 0]] * pw[1][:, ex[:, 1]] * pw[2][:, ex[:, 2]]


def _offsets(pts, centres, labels, inv):
    """The kernels' scaled offsets and their squared lengths, float32 operation by operation."""
    d = (pts - centres[labels]) * inv
    r2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    return d, r2


# ---- the references ----
def _model(pts, labels, K, weights, inv, p, C, ex, abs_extra=None, drop=None, h64=None, centres=None):
    """Per cell k and monomial t, float64: value coefficients C_t sum w e dx^t (columns of weights), the absolute set C_t sum |w| e |dx^t|,
    the conditioning set (|w| |dx|^2) and, if given, the set with weights abs_extra (|w| eps).  -> dict of (K, pd, ncol) arrays."""
    pd = len(ex)
    nw = weights.shape[1]
    out = {q: np.zeros((K, pd, nw)) for q in ("val", "abs", "cond", "eps")}
    wv = weights.copy()
    if drop is not None:
        wv[drop] = 0.0
    order = np.argsort(labels, kind="stable")
    bounds = np.searchsorted(labels[order], np.arange(K + 1))
    step = max(256, (1 << 21) // pd)
    for k in range(K):
        for lo in range(bounds[k], bounds[k + 1], step):
            mem = order[lo:min(bounds[k + 1], lo + step)]
            if h64 is None:
                d, r2 = _offsets(pts[mem], centres, labels[mem], inv)
                d64, r64 = d.astype(np.float64), r2.astype(np.float64)
            else:                                  # mutation: the exact 1 / sqrt(2 sigma^2) in place of the float32 inv
                d64 = (pts[mem] - centres[labels[mem]]).astype(np.float64) * h64
                r64 = (d64 * d64).sum(axis=1)
            with np.errstate(over="ignore", invalid="ignore"):
                e = np.exp(-r64)
                mono = _mono(d64, ex)
                mono = np.where(e[:, None] == 0.0, 0.0, mono)     # (0 * d^t: the recursion starts from the seed and never forms d^t alone)
            w = weights[mem]
            sets = {"val": wv[mem] * e[:, None], "abs": np.abs(w) * e[:, None], "cond": np.abs(w) * (e * r64)[:, None]}
            if abs_extra is not None:
                sets["eps"] = abs_extra[mem] * e[:, None]
            amono = np.abs(mono)
            for q, s in sets.items():
                out[q][k] += (mono if q == "val" else amono).T @ s
    for q in out:
        out[q] *= C[None, :, None]
    return out


def _reach(q, centres, inv, e):
    """(K, nq) mask of the pairs the predict kernel evaluates: NOT (|dy|^2 > e) on the float32 bits (a NaN mean is reached)."""
    K = len(centres)
    reach = np.zeros((K, len(q)), bool)
    for k in range(K):
        _, r2 = _offsets(q, centres[k:k + 1], np.zeros(len(q), np.int64), inv)
        reach[k] = ~(r2 > f32(e))
    return reach


def _predict(q, centres, coef, inv, e, ex, reach, skip=None, h64=None):
    """v[q, col] = sum_{k in reach} e^{-|dy|^2} sum_t coef dy^t for every coefficient set; plus sum e |dy|^2 (|mono| . abs) for the
    conditioning of B, the number of cells in reach and the members behind them."""
    nq = len(q)
    res = {s: np.zeros((nq, coef[s].shape[2])) for s in coef}
    res["abs_dy2"] = np.zeros((nq, coef["abs"].shape[2]))
    for k in range(len(centres)):
        idx = np.nonzero(reach[k])[0]
        if len(idx) == 0:
            continue
        if h64 is None:
            d, r2 = _offsets(q[idx], centres[k:k + 1], np.zeros(len(idx), np.int64), inv)
            d64, r64 = d.astype(np.float64), r2.astype(np.float64)
        else:
            d64 = (q[idx] - centres[k]).astype(np.float64) * h64
            r64 = (d64 * d64).sum(axis=1)
        ek = np.exp(-r64)
        mono = _mono(d64, ex)
        amono = np.abs(mono)
        if skip is not None and skip[1] == k:
            ek_val = np.where(idx == skip[0], 0.0, ek)
        else:
            ek_val = ek
        for s in coef:
            if s == "val":
                res[s][idx] += ek_val[:, None] * (mono @ coef[s][k])
            else:
                res[s][idx] += ek[:, None] * (amono @ coef[s][k])
        res["abs_dy2"][idx] += (ek * r64)[:, None] * (amono @ coef["abs"][k])
    return res


def _closed_form(q, pts, labels, centres, weights, inv, p, reach, max_pairs):
    """Reference B of one transform: sum over the members of the reached cells of w exp(-|dx|^2 - |dy|^2 + 2 dx.dy), and the Taylor
    remainder allowance of those pairs.  None if more than max_pairs pairs are in reach."""
    K = len(centres)
    order = np.argsort(labels, kind="stable")
    bounds = np.searchsorted(labels[order], np.arange(K + 1))
    pairs = sum(int(reach[k].sum()) * int(bounds[k + 1] - bounds[k]) for k in range(K))
    if pairs > max_pairs:
        return None
    nq, nw = len(q), weights.shape[1]
    val, rem = np.zeros((nq, nw)), np.zeros((nq, nw))
    lgp = math.lgamma(p + 1)
    for k in range(K):
        idx = np.nonzero(reach[k])[0]
        mem = order[bounds[k]:bounds[k + 1]]
        if len(idx) == 0 or len(mem) == 0:
            if len(idx) and not np.isfinite(centres[k]).all():
                val[idx] = np.nan
            continue
        dx, _ = _offsets(pts[mem], centres, labels[mem], inv)
        dx = dx.astype(np.float64)
        rx = (dx * dx).sum(axis=1)
        ax = np.sqrt(rx)
        w = weights[mem]
        step = max(1, (1 << 22) // len(mem))
        for lo in range(0, len(idx), step):
            qi = idx[lo:lo + step]
            dy, _ = _offsets(q[qi], centres[k:k + 1], np.zeros(len(qi), np.int64), inv)
            dy = dy.astype(np.float64)
            ry = (dy * dy).sum(axis=1)
            ex = -(ry[:, None] + rx[None, :]) + 2.0 * (dy @ dx.T)
            val[qi] += np.exp(ex) @ w
            t = 2.0 * np.sqrt(ry)[:, None] * ax[None, :]
            with np.errstate(divide="ignore"):
                lr = -(ry[:, None] + rx[None, :]) + t + p * np.log(t) - lgp
            rem[qi] += np.exp(lr) @ np.abs(w)
    return val, rem


def references(case, drop=None, swap_c=None, order_minus_one=False, skip=None, h64=False, max_pairs=B_MAX_PAIRS, kcenter=None,
               ck=None, with_b=True):
    """{"A": r, "B": r or None}: P1, Pt1, PX, L and their bounds.  Mutations of A (the comparator must reject them): drop = (side, point)
    leaves one member out of its cell's coefficients (side "y": Kt1's model, "x": P1 / PX's); swap_c = (t1, t2) swaps two C_a; order_minus_one
    evaluates at p - 1; skip = (side, query, cell) leaves one reached cell out of one query; h64 uses the float64 1 / sqrt(2 sigma^2)."""
    y, x, m, n = case.y, case.x, case.m, case.n
    p = case.p - 1 if order_minus_one else case.p
    K = cluster_count(m, n, case.sigma2, case.sigma2_init)
    _, inv = hsigma_inv(case.sigma2)
    h = 1.0 / math.sqrt(2.0 * float(f32(case.sigma2))) if h64 else None
    nd = ndi(case.sigma2, case.weight, m, n)
    ex = exponents(p)
    C = ck(p).astype(np.float64)
    if swap_c is not None:
        C[[swap_c[0], swap_c[1]]] = C[[swap_c[1], swap_c[0]]]
    xc_y, lab_y = kcenter(y, K)
    xc_x, lab_x = kcenter(x, K)
    lab_y, lab_x = lab_y.astype(np.int64), lab_x.astype(np.int64)
    pdv = len(ex)
    cy = np.bincount(lab_y, minlength=K)
    cx = np.bincount(lab_x, minlength=K)
    # Kt1: the moving cloud, unit weights, queried at the fixed cloud
    By = _model(y, lab_y, K, np.ones((m, 1)), inv, p, C, ex, drop=drop[1] if drop and drop[0] == "y" else None, h64=h, centres=xc_y)
    reach_x = _reach(x, xc_y, inv, case.e)
    kt = _predict(x, xc_y, By, inv, case.e, ex, reach_x, skip=skip[1:] if skip and skip[0] == "y" else None, h64=h)
    # P1 / PX: the fixed cloud weighted by 1/den and x/den, queried at the moving cloud
    reach_y = _reach(y, xc_x, inv, case.e)
    pl = plan(case)
    out = {}
    depth_common = (p + 2) + 2 * max(p - 1, 0)
    b_kt = None
    if with_b and not (drop or swap_c or order_minus_one or skip or h64):
        b_kt = _closed_form(x, y, lab_y, xc_y, np.ones((m, 1)), inv, p, reach_x, max_pairs)
    for var in ("A", "B"):
        if var == "B" and b_kt is None:
            out["B"] = None
            continue
        kt1 = kt["val"][:, 0] if var == "A" else b_kt[0][:, 0]
        den = kt1 + nd
        flush_scale = FLT_MIN * pdv * 8.0 * max(1.0, case.e) ** (max(p - 1, 0) / 2.0)
        nreach_y = reach_x.sum(axis=0)
        members_x = (reach_x * cy[:, None]).sum(axis=0)
        dmodel_y = _model_depth(cy, pl["Zy"])
        depth_kt = dmodel_y + depth_common + (K + pl["Sa"] - 1) // pl["Sa"] + pl["Sa"]
        kt_norm = U * (4 + math.sqrt(depth_kt)) * kt["abs"][:, 0] + flush_scale * (members_x + nreach_y)
        if var == "B":
            kt_norm = kt_norm + 3 * U * (kt["cond"][:, 0] + kt["abs_dy2"][:, 0]) + b_kt[1][:, 0]
        aden = np.abs(den)
        eps_x = kt_norm / aden + U
        pt1 = 1.0 - nd / den
        qq = nd / aden
        pt1_norm = qq * kt_norm / aden + 2 * U * (1 + qq)
        w = np.column_stack([x.astype(np.float64) / den[:, None], 1.0 / den])            # (x/den, y/den, z/den, 1/den): xw4
        Bx = _model(x, lab_x, K, w, inv, p, C, ex, abs_extra=np.abs(w) * eps_x[:, None], drop=drop[1] if drop and drop[0] == "x" else None,
                    h64=h, centres=xc_x)
        v = _predict(y, xc_x, Bx, inv, case.e, ex, reach_y, skip=skip[1:] if skip and skip[0] == "x" else None, h64=h)
        nreach = reach_y.sum(axis=0)
        members_y = (reach_y * cx[:, None]).sum(axis=0)
        dmodel_x = _model_depth(cx, pl["Za"])
        depth_v = dmodel_x + depth_common + (K + pl["Sy"] - 1) // pl["Sy"] + pl["Sy"]
        maxw = float(np.nanmax(np.abs(w))) if np.isfinite(w).any() else 0.0
        v_norm = U * (4 + math.sqrt(depth_v)) * v["abs"] + v["eps"] + (flush_scale * (1 + maxw) * (members_y + nreach))[:, None]
        vals = v["val"]
        if var == "B":
            bv = _closed_form(y, x, lab_x, xc_x, w, inv, p, reach_y, max_pairs)
            if bv is None:
                out["B"] = None
                continue
            vals = bv[0]
            v_norm = v_norm + 3 * U * (v["cond"] + v["abs_dy2"]) + bv[1]
        logs = np.log(aden)
        with np.errstate(invalid="ignore"):
            L = -float(np.log(den).sum()) + 1.5 * n * math.log(float(f32(case.sigma2)))
        L_norm = float((kt_norm / aden + 4 * U + U * np.abs(logs)).sum()) + U * (abs(L) + 2 * abs(1.5 * n * math.log(case.sigma2)))
        r = dict(p1=vals[:, 3], px=vals[:, :3], pt1=pt1, L=L, p1_norm=v_norm[:, 3], px_norm=v_norm[:, :3], pt1_norm=pt1_norm, L_norm=L_norm,
                 kt1=kt1, K=K, n=n, m=m, sum_abs_log=float(np.abs(logs).sum()), maxcell=int(max(cy.max(), cx.max())), remainder_vacuous=False, depth=(depth_kt, depth_v))
        if var == "B":
            r["remainder_vacuous"] = bool((b_kt[1][:, 0] > kt["abs"][:, 0]).any() or (bv[1] > v["abs"]).any())
        out[var] = r
    return out


def _model_depth(counts, Z):
    """The longest fp32 chain of a cell's coefficient: a group's members (tiles g, g + G, ... of its share of the Z splits), the G group
    adds, the Z partial adds, x C_a."""
    big = int(counts.max()) if len(counts) else 0
    per_split = -(-big // Z)
    per_group = min(per_split, -(-per_split // (FGT_TILE * FGT_MODEL_GROUPS)) * FGT_TILE)
    return per_group + FGT_MODEL_GROUPS + Z + 1


def oracle_depth_extra(r, p):
    """cpu-slam's chains beyond the kernels': every member of a cell in one running sum, every monomial of every reached cell in one."""
    return r["maxcell"] + r["K"] * pd_of(p)


def outputs_of(r):
    """A reference's values rounded to the kernels' output types: the mutation check's stand-in for a kernel."""
    return (r["p1"].astype(np.float32), r["pt1"].astype(np.float32), r["px"].astype(np.float32), float(np.float32(r["L"])))


def ratios(out, r, extra_depth=0, a=None):
    """Per element |out - r| / bound of P1, Pt1, PX and L, each reduced to its maximum and the argmax.  Elements where the reference (or
    reference A, a: the truncated series' NaN, log of a negative den, that B does not have) is NaN are skipped here (the NaN pattern is
    checked on its own, nan_mismatch); a non-finite output where the reference is finite is inf."""
    a = a or r
    p1, pt1, px, L = out
    scale = 1.0
    if extra_depth:
        d = max(r["depth"])
        scale = (4 + math.sqrt(d + extra_depth)) / (4 + math.sqrt(d))
    res = {}
    for key, got, want, norm in (("p1", p1, r["p1"], r["p1_norm"]), ("pt1", pt1, r["pt1"], r["pt1_norm"]), ("px", px, r["px"], r["px_norm"])):
        got = np.asarray(got, np.float64)
        with np.errstate(invalid="ignore"):
            err = np.abs(got - want)
            rr = np.where(err == 0, 0.0, err / np.maximum(norm * scale, 1e-300))
        rr = np.where(np.isnan(want) | np.isnan(a[key]), 0.0, np.where(np.isfinite(got), rr, np.inf))
        i = int(np.argmax(rr)) if rr.size else 0
        res[key] = (float(rr.ravel()[i]) if rr.size else 0.0, i)
    if np.isfinite(r["L"]) and np.isfinite(a["L"]):
        L_norm = r["L_norm"] * scale
        if extra_depth:
            L_norm += U * r["n"] * r["sum_abs_log"]      # (cpu-slam adds the logs in one fp32 running sum: gamma_n, not its square root)
        res["L"] = (abs(float(L) - r["L"]) / L_norm if np.isfinite(L) else math.inf, 0)
    return res


def nan_mismatch(out, r):
    """Elements whose NaN-ness differs between the output and the reference."""
    p1, pt1, px, L = out
    bad = {}
    for key, got, want in (("p1", p1, r["p1"]), ("pt1", pt1, r["pt1"]), ("px", px, r["px"]), ("L", np.float64(L), np.float64(r["L"]))):
        d = np.isnan(np.asarray(got, np.float64)) != np.isnan(want)
        if d.any():
            bad[key] = int(d.sum())
    return bad


def worst(res):
    k = max(res, key=lambda q: res[q][0])
    return res[k][0], k


def kernel_form_coefficient(case, kcenter, ck, side="x"):
    """float32 emulation of the library's model formula before the fix: the member's powers d^0 .. d^(p-1) formed first, then
    ((se * z^c) * y^b) * x^a (cpd_fgt.hip fgt_model_kernel) -- unit weights; -> (K, pd) float32 coefficient sums."""
    pts = case.x if side == "x" else case.y
    K = cluster_count(case.m, case.n, case.sigma2, case.sigma2_init)
    _, inv = hsigma_inv(case.sigma2)
    xc, lab = kcenter(pts, K)
    ex = exponents(case.p)
    d, r2 = _offsets(pts, xc, lab.astype(np.int64), inv)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        se = np.exp(-r2)
        pw = np.ones((3, len(pts), case.p), np.float32)
        for r in range(1, case.p):
            pw[:, :, r] = d.T * pw[:, :, r - 1]
        pr = ((se[:, None] * pw[2][:, ex[:, 2]]) * pw[1][:, ex[:, 1]]) * pw[0][:, ex[:, 0]]
        acc = np.zeros((K, len(ex)), np.float32)
        for k in range(K):
            acc[k] = pr[lab == k].sum(axis=0, dtype=np.float32)
    return acc * ck(case.p)[None, :]


# ---- the mutations the comparator must reject ----
def mutation(case, kind, kcenter):
    """Keyword arguments of references() for one mutation of reference A on this case."""
    from scipy.spatial import cKDTree
    if kind == "drop_member":                   # the fixed point nearest to a moving point: the largest Gaussian of some P1
        d, _ = cKDTree(case.y.astype(np.float64)).query(case.x.astype(np.float64))
        return dict(drop=("x", int(np.argmin(d))))
    if kind == "swap_c":                        # x^2 (C = 2) against xy (C = 4)
        ex = [tuple(e) for e in exponents(case.p)]
        return dict(swap_c=(ex.index((2, 0, 0)), ex.index((1, 1, 0))))
    if kind == "order_minus_one":
        return dict(order_minus_one=True)
    if kind == "skip_cell":                     # Kt1 of the fixed point nearest to a moving point loses the cell of that moving point
        d, j = cKDTree(case.y.astype(np.float64)).query(case.x.astype(np.float64))
        q = int(np.argmin(d))
        K = cluster_count(case.m, case.n, case.sigma2, case.sigma2_init)
        _, lab = kcenter(case.y, K)
        return dict(skip=("y", q, int(lab[j[q]])))
    if kind == "h64":
        return dict(h64=True)
    raise ValueError(kind)


MUTATIONS = ("drop_member", "swap_c", "order_minus_one", "skip_cell", "h64")
