"""A seeded catalogue of CPD E-step problems and two float64 references of the exact and the truncated E-step, with per-element error
bounds.  Shared by tests/test_estep_reference.py (CPU: the bound model against the oracle, the plan coverage, the mutation check) and
tests/test_gpu_estep.py (every case on the VALU / MFMA exact E-step and the culled / every-pair truncated one).  Generated in code: the
same seed gives the same float32 clouds on every machine.

References (both from the same float32 inputs):
  A "kernel exponents": the exponent is formed in float32 exactly as the kernels form it (cpd_kernels.hip sq_dist / affinity: dx = a - y,
    d = (dx dx + dy dy) + dz dz, mult = -0.5f / sigma2, e = mult d -- numpy rounds once per float32 operation); exp, every sum, w and L in
    float64.  The truncation set is decided on those float32 exponents; pairs within 2 ulp of log(truncate) are AMBIGUOUS (the host's logf
    may differ from numpy's by an ulp) and their contribution is added to the allowed error.  What remains is the kernels' exp and sums.
  B "exact": everything in float64.  The float32 exponent's own error (u |e| per rounding, six roundings) is added to the allowed error
    as the conditioning term u sum p (6|e| + 1), propagated into P1 / PX through w.

Bounds, per element, normalised by the sum of the absolute values of the terms (never by an array maximum), u = 2^-24:
  den_x  u (sum_k p_xk + c)            P1_k   u P1_k              PX_kc  u sum_x p_xk w_x |x_c|
  Pt1_x  u (absolute)                  L      sum_x rel.err(den_x) + u (|sum log den| + |1.5 n log sigma2|)
each scaled by (1 + sqrt(depth)), depth = the longest sequential fp32 chain of that element on the path (plan_chunks mirror: chunk length
plus post-kernel chain; a chain adds at most as many non-zero terms as the element has, and adding an exact zero does not round), plus
FLT_MIN per term the kernel may flush to zero.  The bar on |kernel - reference| / normalisation is BAR, fixed before any measurement."""
import math

import numpy as np

U = 2.0 ** -24
FLT_MIN = float(np.finfo(np.float32).tiny)
BAR = 16.0
CU_COUNT = 256                    # MI355X
CPD_T, CPD_MAX_CHUNKS = 8, 256    # cpd_kernels.h
TRUNC_TILE, TRUNC_GROUP = 64, 16
TRUNC_MAX_BLOCKS = 4096
UNDERFLOW_E = -104.0              # exp(e) < 2^-150 below this: the kernel's affinity is exactly 0
SPARSE_E = -110.0                 # sparse references drop pairs below this exponent (each < 2e-48: inside the FLT_MIN allowance)
WEIGHTS = (1e-6, 0.3, 1.0 - 1e-6)
PATHS = ("valu", "mfma", "culled", "every_pair")


# ---- the plan (cpd_plan.hpp plan_chunks, cpd_chunk_plan; tests/test_cpd_plan.py holds the two together) ----
def plan_chunks(owners, owner_r, stream_len, cu_count=CU_COUNT):
    owner_blocks = max(1, (owners + 256 * owner_r - 1) // (256 * owner_r))
    ch = (cu_count * 8 + owner_blocks - 1) // owner_blocks
    ch = max(1, min(ch, min(CPD_MAX_CHUNKS, max(1, stream_len // (CPD_T * 8)))))
    chunk_len = ((stream_len + ch - 1) // ch + CPD_T - 1) // CPD_T * CPD_T
    return (stream_len + chunk_len - 1) // chunk_len, chunk_len


def plan(m, n, cu_count=CU_COUNT):
    """K7a (owners: the n fixed points, 4 per lane; stream: the m moving points) and K7b (owners: moving points, 2 per lane; stream: fixed
    points): chunk count, chunk length, last-chunk length; MFMA blocks of CPD_T fixed points in each K7b chunk; the truncated tiles."""
    kc, kl = plan_chunks(n, 4, m, cu_count)
    xc, xl = plan_chunks(m, 2, n, cu_count)
    x_last = n - (xc - 1) * xl
    return dict(k_chunks=kc, k_chunk_len=kl, k_last=m - (kc - 1) * kl, x_chunks=xc, x_chunk_len=xl, x_last=x_last,
                mfma_blocks=sorted({x_last // CPD_T} | ({xl // CPD_T} if xc > 1 else set())),
                tiles_m=(m + TRUNC_TILE - 1) // TRUNC_TILE, tiles_n=(n + TRUNC_TILE - 1) // TRUNC_TILE)


def depths(m, n, path, cu_count=CU_COUNT):
    """(chain, post) of the denominators and of the contraction on `path`: `chain` sequential fp32 adds of pair terms, then `post` adds of
    partial sums (and of c).  oracle: cpu-slam's one running sum per element."""
    if path == "oracle":
        return (m, 1), (n, 0)
    if path == "culled":
        # a wave adds its groups (round-robin over 4 waves) in order, the four wave sums are added in wave order (cpd_trunc.hip)
        return (TRUNC_GROUP * ((m + TRUNC_TILE - 1) // TRUNC_TILE), 4), (TRUNC_GROUP * ((n + TRUNC_TILE - 1) // TRUNC_TILE), 3)
    p = plan(m, n, cu_count)
    # a chunk's sum, then a quarter of the chunk partials per lane of a quad, the quad's 3 adds (+ c for the denominators)
    return (p["k_chunk_len"], (p["k_chunks"] + 3) // 4 + 4), (p["x_chunk_len"], (p["x_chunks"] + 3) // 4 + 3)


# ---- the catalogue ----
class Case:
    def __init__(self, name, cls, y, x, sigma2, weight, truncate=1e-3, exact=True, sparse=False, big=False):
        self.name, self.cls = name, cls
        self.y, self.x = np.ascontiguousarray(y, np.float32), np.ascontiguousarray(x, np.float32)
        self.sigma2 = float(np.float32(sigma2))
        self.weight = weight
        self.truncate = truncate
        self.exact = exact            # also run on the exact E-step (the truncated-only classes are not)
        self.sparse = sparse          # reference from the pairs in reach (k-d tree): every other pair's exponent is below SPARSE_E / the cut
        self.big = big                # reference too slow for the CPU suite
        self.constant = None

    @property
    def m(self):
        return len(self.y)

    @property
    def n(self):
        return len(self.x)

    def __repr__(self):
        return "%s(%d x %d, sigma2 %g, w %g)" % (self.name, self.m, self.n, self.sigma2, self.weight)


def _uniform(rng, k, half=5.0):
    return rng.uniform(-half, half, (k, 3))


def _near(rng, base, k, scale=0.2):
    return base[rng.integers(0, len(base), k)] + rng.normal(scale=scale, size=(k, 3))


def _lattice(k, spacing=1.0, planar=False):
    side = int(math.ceil(k ** (0.5 if planar else 1.0 / 3.0)))
    g = np.arange(side, dtype=np.float64) * spacing
    if planar:
        pts = np.stack(np.meshgrid(g, g, [0.0], indexing="ij"), -1).reshape(-1, 3)
    else:
        pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    return pts[:k]


def _rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    return q if np.linalg.det(q) > 0 else -q


def catalogue(seed=20261016, with_big=True):
    """Every case of the catalogue (constants still unset: attach_constants, which needs the oracle)."""
    rng = np.random.default_rng(seed)
    cases = []
    wi = [0]

    def add(name, cls, y, x, sigma2, **kw):
        cases.append(Case(name, cls, y, x, sigma2, WEIGHTS[wi[0] % 3], **kw))
        wi[0] += 1

    # uniform: a tail-loop-only K7a (m < 8), one MFMA block (8 <= n < 16), and the ragged sizes
    y = _uniform(rng, 5); add("uniform_5x300", "uniform", y, _near(rng, y, 300, 1.0), 2.0)
    y = _uniform(rng, 65); add("uniform_65x9", "uniform", y, _near(rng, y, 9, 0.5), 1.0)
    y = _uniform(rng, 257); add("uniform_257x1025", "uniform", y, _near(rng, y, 1025), 0.5)
    y = _uniform(rng, 320); add("uniform_320x1024", "uniform", y, _near(rng, y, 1024), 0.3)
    y = _uniform(rng, 4097); add("uniform_4097x4099", "uniform", y, _near(rng, y, 4099), 0.05)
    # the 256-chunk cap on either side: 100 000 x 7 and 7 x 100 000
    y = _uniform(rng, 100000); add("uniform_100000x7", "uniform", y, _near(rng, y, 7, 0.1), 0.02)
    y = _uniform(rng, 7); add("uniform_7x100000", "uniform", y, _near(rng, y, 100000, 2.0), 1.5)
    # clustered blobs; a K7a last chunk of one point (2305 = 32 x 72 + 1)
    centres = _uniform(rng, 12)
    y = _near(rng, centres, 2305, 0.3); add("blobs_2305x2047", "blobs", y, _near(rng, centres, 2047, 0.3), 0.1)
    y = _near(rng, centres, 577, 0.3); add("blobs_577x1009", "blobs", y, _near(rng, centres, 1009, 0.3), 0.05)
    # exactly planar clouds (z = 0)
    y = _uniform(rng, 319); y[:, 2] = 0
    x = _near(rng, y, 2047, 0.3); x[:, 2] = 0
    add("planar_319x2047", "planar", y, x, 0.2)
    # integer lattice: exact distance ties
    y = _lattice(321); add("lattice_321x1025", "lattice", y, _lattice(1025) - 1.0, 0.7)
    # duplicated points, y = x exactly: exponent 0, p = 1
    y = _uniform(rng, 511); y[256:300] = y[0]
    add("duplicate_511x511", "duplicate", y, y.copy(), 0.1)
    # offset by 1e3
    y = _uniform(rng, 767) + 1e3; add("offset_767x2047", "offset", y, _near(rng, y, 2047), 0.1)
    # 5 % far outliers on both sides (their Pt1 / P1 / PX: exactly 0)
    y = _uniform(rng, 2049); x = _near(rng, y, 1025)
    y[rng.permutation(2049)[:102]] += 1e4; x[rng.permutation(1025)[:51]] -= 1e4
    add("outliers_2049x1025", "outliers", y, x, 0.3)
    # sigma^2 from nearly everything underflowing to everything ~ 1
    y = _uniform(rng, 1023); x = _near(rng, y, 1025, 1.0)
    for s2 in (0.004, 0.05, 5.0, 1e4):
        add("sigma2_%g_1023x1025" % s2, "sigma2", y, x, s2)
    # long MFMA chunks: 100 000 x 45 000 plans 11 K7b chunks of 4 096 points (512 blocks); at this sigma^2 next to every pair underflows,
    # so the pairs in reach are all the reference needs
    y = _uniform(rng, 100000, 20.0); add("underflow_100000x45000", "sigma2", y, _near(rng, y, 45000, 0.3), 0.01, sparse=True)
    # -- truncated only --
    # sparse: a few pairs in reach; more than 4 096 tiles on both sides (the owner loops of cpd_trunc.hip)
    y = _uniform(rng, 270001, 60.0); x = np.concatenate([_near(rng, y[:200000], 200000, 0.05), _uniform(rng, 70017, 60.0)])
    add("sparse_270001x270017", "sparse", y, x, 0.002, exact=False, sparse=True)
    y = _uniform(rng, 4159, 30.0); add("sparse_4159x3135", "sparse", y, _near(rng, y, 3135, 0.1), 0.01, exact=False)
    # a lattice whose spacing is the truncation radius sqrt(-2 sigma^2 ln t): every neighbour on the boundary
    s2 = 0.1
    h = float(np.float32(math.sqrt(-2.0 * s2 * math.log(1e-3))))
    y = _lattice(1000, h); add("radius_lattice_1000x1000", "radius_lattice", y, y.copy(), s2, exact=False)
    # the moving cloud rotated and translated away from the curve order the culled kernel tiles by
    y = _near(rng, _uniform(rng, 30), 3001, 0.5)
    x = _near(rng, y, 2993, 0.05) @ _rotation(rng).T + np.array([0.3, -0.2, 0.1])
    add("moved_3001x2993", "moved", y @ _rotation(rng).T + 0.7, x, 0.02, exact=False)
    if with_big:
        # the size the reference publishes for CPD (dense: every pair contributes)
        y = _uniform(rng, 49000); add("dense_49000x49000", "uniform", y, _near(rng, y, 49000), 0.5, big=True)
    return cases


def attach_constants(cases, cpd_constant):
    """c = oracle.cpd_constant(sigma2, weight, m, n) (coherentpointdrift.cpp:98)."""
    for c in cases:
        c.constant = float(np.float32(cpd_constant(c.sigma2, c.weight, c.m, c.n)))
    return cases


def coverage(cases, cu_count=CU_COUNT):
    """What the catalogue's shapes reach of the plan, per requirement -> the cases that reach it."""
    cov = {}

    def hit(key, case):
        cov.setdefault(key, []).append(case.name)
    for c in cases:
        m, n = c.m, c.n
        if c.exact:
            p = plan(m, n, cu_count)
            if p["k_chunks"] == 1 and m < CPD_T:
                hit("k_chunks=1,m<8", c)
            if p["k_chunks"] == CPD_MAX_CHUNKS:
                hit("k_chunks=256", c)
            if p["x_chunks"] == CPD_MAX_CHUNKS:
                hit("x_chunks=256", c)
            if (p["k_chunks"] > 1 and p["k_last"] < CPD_T) or (p["x_chunks"] > 1 and p["x_last"] < CPD_T):
                hit("last_chunk<8", c)
            for b in p["mfma_blocks"]:
                if b == 0:
                    hit("mfma_blocks=0", c)
                if b == 1:
                    hit("mfma_blocks=1", c)
                if b >= 2 and b % 2 == 0:
                    hit("mfma_blocks_even", c)
                if b >= 3 and b % 2 == 1:
                    hit("mfma_blocks_odd>=3", c)
                if b >= 500:
                    hit("mfma_blocks>=500", c)
        for r in (1, 63, 64, 65, 255):
            if m % 256 == r:
                hit("m%%256=%d" % r, c)
        for r in (1, 1023):
            if n % 1024 == r:
                hit("n%%1024=%d" % r, c)
        for r in (1, 63):
            if m % TRUNC_TILE == r or n % TRUNC_TILE == r:
                hit("tiles%%64=%d" % r, c)
        if (m + TRUNC_TILE - 1) // TRUNC_TILE > TRUNC_MAX_BLOCKS and (n + TRUNC_TILE - 1) // TRUNC_TILE > TRUNC_MAX_BLOCKS:
            hit("tiles>4096", c)
    return cov


REQUIRED_COVERAGE = ("k_chunks=1,m<8", "k_chunks=256", "x_chunks=256", "last_chunk<8", "mfma_blocks=0", "mfma_blocks=1", "mfma_blocks_even",
                     "mfma_blocks_odd>=3", "mfma_blocks>=500", "m%256=1", "m%256=63", "m%256=64", "m%256=65", "m%256=255", "n%1024=1",
                     "n%1024=1023", "tiles%64=1", "tiles%64=63", "tiles>4096")


# ---- the references ----
def _ulp32(v):
    return float(np.spacing(np.float32(abs(v))))


def _pairs(case, cut_e):
    """Sparse cases: (row, col) of every pair whose float64 exponent lies above cut_e (a k-d tree query), rows ascending."""
    from scipy.spatial import cKDTree
    radius = math.sqrt(cut_e / (0.5 / case.sigma2)) * (1.0 + 1e-5)
    sm = cKDTree(case.x.astype(np.float64)).sparse_distance_matrix(cKDTree(case.y.astype(np.float64)), radius, output_type="coo_matrix")
    order = np.argsort(sm.row, kind="stable")
    return sm.row[order].astype(np.int64), sm.col[order].astype(np.int64)


def _block(case, lo, hi, rc, modes, lt32, band32, drop):
    """The float64 sums of fixed points [lo, hi) against every moving point (dense) or the pairs rc (sparse): per (mode, variant) the
    rows' den / counts / ambiguous / conditioning sums and the columns' contraction."""
    import scipy.sparse as sp
    y, x, m, c = case.y, case.x, case.m, float(case.constant)
    nb = hi - lo
    s2 = np.float32(case.sigma2)
    mult32, mult64 = np.float32(-0.5) / s2, -0.5 / float(s2)
    if rc is None:
        d32 = [x[lo:hi, i][:, None] - y[None, :, i] for i in range(3)]
        d64 = [x[lo:hi, i].astype(np.float64)[:, None] - y[None, :, i].astype(np.float64) for i in range(3)]
        rowsum = lambda v: v.sum(axis=1)                                                     # noqa: E731
        colcount = lambda b: np.count_nonzero(b, axis=0)                                      # noqa: E731
        rowcount = lambda b: np.count_nonzero(b, axis=1)                                      # noqa: E731
        tmul = lambda v, W: v.T @ W                                                           # noqa: E731
    else:
        rr, cc = rc
        rl = rr - lo
        indptr = np.searchsorted(rl, np.arange(nb + 1))
        d32 = [x[rr, i] - y[cc, i] for i in range(3)]
        d64 = [x[rr, i].astype(np.float64) - y[cc, i].astype(np.float64) for i in range(3)]
        rowsum = lambda v: np.bincount(rl, v, nb)                                             # noqa: E731
        colcount = lambda b: np.bincount(cc[b], minlength=m)                                  # noqa: E731
        rowcount = lambda b: np.bincount(rl[b], minlength=nb)                                 # noqa: E731
        tmul = lambda v, W: sp.csr_matrix((v, cc, indptr), shape=(nb, m)).T @ W               # noqa: E731
    # A: the kernels' float32 exponent, one rounding per operation (numpy float32 arithmetic); B: the same in float64
    e32 = mult32 * ((d32[0] * d32[0] + d32[1] * d32[1]) + d32[2] * d32[2])
    e64 = mult64 * ((d64[0] * d64[0] + d64[1] * d64[1]) + d64[2] * d64[2])
    del d32, d64
    eA = e32.astype(np.float64)
    pA, pB = np.exp(eA), np.exp(e64)
    if drop is not None and lo <= drop[0] < hi:
        if rc is None:
            pA[drop[0] - lo, drop[1]] = 0.0
        else:
            pA = np.where((rr == drop[0]) & (cc == drop[1]), 0.0, pA)
    live = e32 > UNDERFLOW_E
    xb = x[lo:hi].astype(np.float64)
    out = {}
    for mode in modes:
        if mode == "trunc":
            keepA, keepB = e32 >= lt32, e64 >= math.log(case.truncate)
            ambA = np.abs(eA - float(lt32)) <= band32
            ambB = np.abs(e64 - math.log(case.truncate)) <= band32 + 8 * U * np.abs(e64)
        for var in ("A", "B"):
            p, e = (pA, eA) if var == "A" else (pB, e64)
            amb = None
            nz = live
            if mode == "trunc":
                keep = keepA if var == "A" else keepB
                amb = np.where(ambA if var == "A" else ambB, np.exp(e), 0.0)
                p = np.where(keep, p, 0.0)
                nz = live & keep
            q = p * (6.0 * np.abs(e) + 1.0) * U if var == "B" else None
            den = rowsum(p) + c
            r = dict(den=den, cnt=rowcount(nz), cntk=colcount(nz), amb=rowsum(amb) if amb is not None else np.zeros(nb),
                     cond=rowsum(q) if q is not None else np.zeros(nb))
            w = 1.0 / den
            extra = (r["amb"] + r["cond"] + m * FLT_MIN) / den                   # den_x's allowance beyond its chain, relative
            wabs = np.column_stack([w, w[:, None] * np.abs(xb)])
            W = np.column_stack([w, w[:, None] * xb, wabs[:, 1:], wabs * extra[:, None]])
            C = tmul(p, W)
            r["P"], r["absPX"], r["extraP"] = C[:, :4], C[:, 4:7], C[:, 7:]
            r["ambP"] = tmul(amb, wabs) if amb is not None else 0.0
            r["condP"] = tmul(q, wabs) if q is not None else 0.0
            out[mode, var] = r
    return lo, hi, out


def references(case, modes=("exact", "trunc"), drop=None, block_pairs=1 << 21, workers=None):
    """{mode: {"A": r, "B": r}} for mode "exact" and / or "trunc" (the truncated E-step at case.truncate).  drop = (x index, k index):
    that pair's term is left out of reference A (the mutation check).  Row blocks of fixed points, on a few threads (numpy releases the
    interpreter in its array operations)."""
    import concurrent.futures
    import os
    m, n, c = case.m, case.n, float(case.constant)
    lt32 = np.float32(np.log(np.float32(case.truncate)))
    band32 = 2.0 * _ulp32(lt32)
    if case.sparse:
        cut = -SPARSE_E if "exact" in modes else -float(lt32) * (1.0 + 1e-3) + band32
        rows, cols = _pairs(case, cut)
        edges = sorted(set(range(0, n, max(1, n // 32))) | {n})
        jobs = []
        for lo, hi in zip(edges[:-1], edges[1:]):
            a, b = np.searchsorted(rows, lo), np.searchsorted(rows, hi)
            jobs.append((lo, hi, (rows[a:b], cols[a:b])))
    else:
        step = max(1, block_pairs // m)
        jobs = [(lo, min(n, lo + step), None) for lo in range(0, n, step)]
    acc = {}
    workers = workers or max(1, min(8, os.cpu_count() or 1, len(jobs)))
    with concurrent.futures.ThreadPoolExecutor(workers) as pool:
        for lo, hi, out in pool.map(lambda j: _block(case, j[0], j[1], j[2], modes, lt32, band32, drop), jobs):
            for key, r in out.items():
                a = acc.setdefault(key, dict(den=np.zeros(n), cnt=np.zeros(n), amb=np.zeros(n), cond=np.zeros(n), P=np.zeros((m, 4)),
                                             absPX=np.zeros((m, 3)), extraP=np.zeros((m, 4)), ambP=np.zeros((m, 4)),
                                             condP=np.zeros((m, 4)), cntk=np.zeros(m)))
                for q in ("den", "cnt", "amb", "cond"):
                    a[q][lo:hi] = r[q]
                for q in ("P", "absPX", "extraP", "ambP", "condP", "cntk"):
                    a[q] += r[q]
    res = {}
    for (mode, var), a in acc.items():
        den = a["den"]
        r = dict(den=den, cnt=a["cnt"], amb=a["amb"], cond=a["cond"], p1=a["P"][:, 0], px=a["P"][:, 1:], absPX=a["absPX"],
                 cntk=a["cntk"], ambP=a["ambP"], extraP=a["extraP"], condP=a["condP"], pt1=1.0 - c / den, c=c, m=m, n=n,
                 sigma2=case.sigma2, maxw=float((1.0 / den).max()), maxabs=float(np.abs(case.x).max()))
        r["L"] = -np.log(den).sum() + 1.5 * n * math.log(case.sigma2)
        res.setdefault(mode, {})[var] = r
    return res


def outputs_of(r):
    """A reference's values rounded to the kernels' output types (p1, pt1, px, L): the mutation check's stand-in for a kernel."""
    return (r["p1"].astype(np.float32), r["pt1"].astype(np.float32), r["px"].astype(np.float32), float(np.float32(r["L"])))


def ratios(out, r, path, cu_count=CU_COUNT):
    """Per-element |out - r| / normalisation of P1, Pt1 (den through it), PX and L, each reduced to its maximum and the argmax."""
    p1, pt1, px, L = out
    m, n, c = r["m"], r["n"], r["c"]
    (dch, dpost), (kch, kpost) = depths(m, n, path, cu_count)
    depth_den = np.minimum(dch, r["cnt"]) + np.minimum(dpost, r["cnt"]) + 1
    den_norm = U * (1 + np.sqrt(depth_den)) * r["den"]                      # (the terms are positive: their sum is den)
    den_extra = r["amb"] + r["cond"] + m * FLT_MIN
    # Pt1 = 1 - c / den: d Pt1 = (c / den) d den / den, plus two roundings
    q = c / r["den"]
    pt1_norm = U * (1 + np.sqrt(depth_den)) + q * den_extra / r["den"]
    # P1 / PX: the contraction's chain plus the denominators' (through w)
    depth_k = np.minimum(kch, r["cntk"]) + np.minimum(kpost, r["cntk"]) + depth_den.max()
    flush = n * FLT_MIN * (1.0 + r["maxw"] * max(1.0, r["maxabs"]))
    p1_norm = U * (1 + np.sqrt(depth_k)) * r["p1"] + r["ambP"][:, 0] + r["extraP"][:, 0] + r["condP"][:, 0] + flush
    px_norm = U * (1 + np.sqrt(depth_k))[:, None] * r["absPX"] + r["ambP"][:, 1:] + r["extraP"][:, 1:] + r["condP"][:, 1:] + flush
    logs = np.log(r["den"])
    L_norm = float((den_norm / r["den"] + den_extra / r["den"]).sum()
                   + U * (3 * n + np.abs(logs).sum() + abs(logs.sum()) + abs(1.5 * n * math.log(r["sigma2"]))))
    if path == "oracle":
        L_norm += U * (1 + math.sqrt(n)) * float(np.abs(logs).sum())          # (cpu-slam adds the logs in one fp32 running sum)
    res = {}
    for key, got, want, norm in (("p1", p1, r["p1"], p1_norm), ("pt1", pt1, r["pt1"], pt1_norm), ("px", px, r["px"], px_norm)):
        err = np.abs(np.asarray(got, np.float64) - want)
        rr = np.where(err == 0, 0.0, err / np.maximum(norm, 1e-300))
        rr = np.where(np.isfinite(np.asarray(got, np.float64)), rr, np.inf)
        i = int(np.argmax(rr)) if rr.size else 0
        res[key] = (float(rr.ravel()[i]) if rr.size else 0.0, i)
    res["L"] = (abs(float(L) - float(r["L"])) / L_norm, 0)
    return res


def worst(res):
    """(largest ratio, quantity)."""
    k = max(res, key=lambda q: res[q][0])
    return res[k][0], k


def out_of_reach(case, truncate):
    """Fixed points with no term in reach: the exponent to every moving point below the truncation band / the underflow threshold."""
    from scipy.spatial import cKDTree
    mult = 0.5 / case.sigma2
    cut = -math.log(case.truncate) * (1.0 + 1e-3) if truncate else -SPARSE_E
    d, _ = cKDTree(case.y.astype(np.float64)).query(case.x.astype(np.float64), k=1)
    return mult * d * d > cut


def mutation_pair(case, mode):
    """The pair the mutation check leaves out of reference A (small dense cases): for the exact E-step the largest term of the fixed point
    with the closest moving point; for the truncated one the kept, unambiguous pair nearest above log(truncate)."""
    y, x = case.y, case.x
    mult32 = np.float32(-0.5) / np.float32(case.sigma2)
    d = [x[:, i][:, None] - y[None, :, i] for i in range(3)]
    e32 = mult32 * ((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    if mode == "exact":
        i = int(np.argmax(e32.max(axis=1)))
        return i, int(np.argmax(e32[i]))
    lt32 = np.float32(np.log(np.float32(case.truncate)))
    e = np.where(e32.astype(np.float64) > float(lt32) + 2.0 * _ulp32(lt32), e32, np.float32(np.inf))
    i, k = np.unravel_index(int(np.argmin(e)), e.shape)
    assert np.isfinite(e[i, k]), "no pair in reach"
    return int(i), int(k)
