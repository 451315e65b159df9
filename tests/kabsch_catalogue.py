"""A seeded catalogue of 3 x 3 cross-covariance matrices for the Kabsch solve (svd3.hpp kabsch_rotation), and the float64 Kabsch
they are measured against.  Shared by tests/test_kabsch3.py (the host IEEE form) and tests/test_gpu_kabsch3.py (both device forms,
through mi_kabsch and mi_cpd_mstep).  Generated in code: the same seed gives the same float32 matrices on every machine."""
import numpy as np

EPS = float(np.finfo(np.float32).eps)
TIE_GAPS = (0.0, 1e-7, 1e-5, 1e-3, 1e-2)          # sigma_2 - sigma_3 relative to sigma_1 of the det < 0 near-ties
SCALES = (("2^100", 2.0 ** 100), ("2^-100", 2.0 ** -100), ("1e30", 1e30), ("1e-30", 1e-30))
WELL_POSED = 1e-4                                 # eps * sigma_1 / g at most: R depends continuously on H
ILL_POSED_GAP = 0.8e-3                            # g below this fraction of sigma_1: R may jump (svd3.hpp hands these to the IEEE form)


def _orthogonal(rng, det):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) * det < 0:
        q[:, 0] = -q[:, 0]
    return q


def _signed_permutations():
    import itertools
    out = []
    for p in itertools.permutations(range(3)):
        for signs in itertools.product((1.0, -1.0), repeat=3):
            m = np.zeros((3, 3))
            for r in range(3):
                m[r, p[r]] = signs[r]
            out.append(m)
    return out                                    # 48: I, -I, diag(1,1,-1), the six permutations, ...


def _usv(rng, s, det_uvt):
    """U diag(s) V^T with random U, V and det(U V^T) = det_uvt."""
    return _orthogonal(rng, 1.0) @ np.diag(s) @ _orthogonal(rng, det_uvt).T


def catalogue(seed=20261016):
    """(H [N, 3, 3] float32, class name per matrix)."""
    rng = np.random.default_rng(seed)
    mats, names = [], []

    def add(name, m):
        mats.append(np.asarray(m, np.float64))
        names.append(name)

    for _ in range(1200):
        add("gaussian", rng.normal(size=(3, 3)))
    for _ in range(900):
        add("rot_diag", _usv(rng, 10.0 ** rng.uniform(-6.0, 0.0, 3), rng.choice((1.0, -1.0))))
    for gap in TIE_GAPS:
        for _ in range(120):
            s2 = rng.uniform(0.05, 0.9)
            add("tie_det_neg_%g" % gap, _usv(rng, (1.0, s2, s2 - gap), -1.0))
    for _ in range(150):
        m = rng.normal(size=(3, 3))
        m[:, rng.integers(3)] = 0.0
        add("rank2", m)
    for _ in range(150):
        add("rank1", np.outer(rng.normal(size=3), rng.normal(size=3)))
    for p in _signed_permutations():
        add("signed_permutation", p)
    for _ in range(100):
        add("rotation", _orthogonal(rng, 1.0))
    for _ in range(100):
        add("reflection", _orthogonal(rng, -1.0))
    for p in _signed_permutations():
        add("near_signed_permutation", p + rng.normal(size=(3, 3)) * 1e-7)
    for _ in range(100):
        add("near_rotation", _orthogonal(rng, rng.choice((1.0, -1.0))) + rng.normal(size=(3, 3)) * 1e-6)
    for name, scale in SCALES:
        for _ in range(75):
            add("scaled_" + name, rng.normal(size=(3, 3)) * scale)
    for side, sign in (("below", -1.0), ("above", 1.0)):
        for _ in range(100):
            s2 = rng.uniform(0.01, 0.9)
            add("threshold_" + side, _usv(rng, (1.0, s2, 1e-3 * (1.0 + sign * 10.0 ** rng.uniform(-3.5, -1.5))), rng.choice((1.0, -1.0))))
    H = np.stack(mats).astype(np.float32)
    assert np.isfinite(H).all() and (np.abs(H)[H != 0] >= np.finfo(np.float32).tiny * 4).all()   # no subnormal entry, none of H / 2 either
    return H, np.array(names)


def kabsch64(H):
    """float64 Kabsch of float32 matrices: (R = U diag(1,1,d) V^T, singular values, d = sign det(U V^T), gap g).  g is the smallest
    pairwise sum of (sigma_1, sigma_2, d sigma_3): R moves by ~ |dH| / g under a change dH."""
    U, S, Vt = np.linalg.svd(np.asarray(H, np.float64))
    d = np.where(np.linalg.det(U @ Vt) < 0, -1.0, 1.0)
    D = np.zeros(U.shape)
    D[:, 0, 0] = D[:, 1, 1] = 1.0
    D[:, 2, 2] = d
    R = U @ D @ Vt
    g = np.minimum(np.minimum(S[:, 0] + S[:, 1], S[:, 0] + d * S[:, 2]), S[:, 1] + d * S[:, 2])
    return R, S, d, g


def posedness(S, g):
    """eps * sigma_1 / g, and the masks (well-posed, ill-posed)."""
    with np.errstate(divide="ignore"):
        cond = np.where(g > 0, EPS * S[:, 0] / np.where(g > 0, g, 1.0), np.inf)
    return cond, cond <= WELL_POSED, g < ILL_POSED_GAP * S[:, 0]


def objective_deficit(R, H, S, d):
    """(sigma_1 + sigma_2 + d sigma_3 - tr(R^T H)) / (sigma_1 + sigma_2 + sigma_3): at most 16 eps for any near-optimal rotation, unique or not."""
    R = np.asarray(R, np.float64)
    tr = np.einsum("nij,nij->n", R, np.asarray(H, np.float64))
    return (S[:, 0] + S[:, 1] + d * S[:, 2] - tr) / S.sum(axis=1)


def orthogonality(R):
    """(max |R^T R - I|, |det R - 1|) per matrix, in float64 of the float32 R."""
    R = np.asarray(R, np.float64)
    e = np.abs(np.einsum("nki,nkj->nij", R, R) - np.eye(3)).max(axis=(1, 2))
    return e, np.abs(np.linalg.det(R) - 1.0)
