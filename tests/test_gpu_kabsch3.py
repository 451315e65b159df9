"""GPU suite: the 3 x 3 Kabsch solve (svd3.hpp kabsch_rotation<true>) matrix by matrix, on the seeded catalogue of tests/kabsch_catalogue.py,
through both of its consumers, in both of its forms (the refined hardware forms of a default context, the IEEE form of a MISLAM_SVD_IEEE=1
context), against float64 and against the oracle (oracle_kabsch_from_h, which the host IEEE form retraces bit for bit: tests/test_kabsch3.py).

Each matrix H reaches the solve exactly:
  * mi_kabsch: source +-e_1, +-e_2, +-e_3 paired with target +-h_c, h = H / 2 -- both centroids are exactly 0 and the fp64 moments sum
    to H without rounding (no catalogue entry of H / 2 is subnormal);
  * mi_cpd_mstep: the same six moving points with P1 = 1 and PX rows +-h_c -- cb = 0, so A = (B^T PX)^T = H exactly.

Then, on every matrix: the IEEE form is the oracle, bit for bit; both forms give a finite, orthogonal R that maximises tr(R^T H); where R is a
continuous function of H both are within 32 (eps sigma_1 / g + eps) of the float64 Kabsch rotation; where it is not (g < 0.8e-3 sigma_1:
mirror ties, rank deficiency) the fast form's R is the IEEE form's, bit for bit -- the policy of the round-5 guard in kabsch_rotation.
"""
import numpy as np
import pytest

from conftest import check_measured
from kabsch_catalogue import EPS, catalogue, kabsch64, objective_deficit, orthogonality, posedness

pytestmark = pytest.mark.gpu

SRC = np.concatenate([np.eye(3), -np.eye(3)]).astype(np.float32)      # +-e_1, +-e_2, +-e_3
IDX = np.arange(6, dtype=np.int32)
ONES6 = np.ones(6, np.float32)
FORMS = ("fast", "ieee")
PATHS = ("kabsch", "mstep")


def moving_images(H):
    """Rows +-h_c (the columns of h = H / 2, exact): paired with SRC their cross-covariance is H."""
    cols = (np.asarray(H, np.float32) * np.float32(0.5)).T
    return np.ascontiguousarray(np.concatenate([cols, -cols]), np.float32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32).reshape(len(a), -1)


@pytest.fixture(scope="module")
def ieee_ctx(capi):
    """A context whose 3 x 3 SVDs run in IEEE divisions and roots (MISLAM_SVD_IEEE=1; switches are read at context creation)."""
    import os
    os.environ["MISLAM_SVD_IEEE"] = "1"
    try:
        c = capi.Context(0)
    finally:
        del os.environ["MISLAM_SVD_IEEE"]
    yield c
    c.close()


class Catalogue:
    def __init__(self, oracle):
        self.H, self.names = catalogue()
        out = [oracle.kabsch_from_h(h) for h in self.H]
        self.R_oracle = np.stack([o[0] for o in out])
        self.R64, self.S64, self.d, self.g = kabsch64(self.H)
        self.cond, self.well, self.ill = posedness(self.S64, self.g)
        e, de = orthogonality(self.R_oracle)
        self.orth_host, self.det_host = e.max(), de.max()              # what the IEEE form reaches on the host (= the oracle's bits)
        self.unscaled = ~np.char.startswith(self.names, "scaled_")      # sigma^2 of these stays inside the fp32 range


@pytest.fixture(scope="module")
def cat(oracle):
    return Catalogue(oracle)


@pytest.fixture(scope="module")
def solved(ctx, ieee_ctx, cat):
    """form -> {"kabsch": R, "mstep": R, "scale": ..., "sigma2": ..., "t_mstep": ...}: one call per matrix and path, computed once."""
    cache = {}

    def get(form):
        if form not in cache:
            c = ctx if form == "fast" else ieee_ctx
            n = len(cat.H)
            out = {"kabsch": np.empty((n, 3, 3), np.float32), "mstep": np.empty((n, 3, 3), np.float32), "t_kabsch": np.empty((n, 3), np.float32),
                   "t_mstep": np.empty((n, 3), np.float32), "scale": np.empty(n), "sigma2": np.empty(n)}
            for i, H in enumerate(cat.H):
                px = moving_images(H)
                R, t, used = c.kabsch(SRC, px, IDX)
                assert used == 6
                out["kabsch"][i], out["t_kabsch"][i] = R, t
                fixed = px if cat.unscaled[i] else SRC                   # (|a|^2 of the 2^100 class would overflow sigma^2's fp32 sum)
                R, t, s, s2 = c.cpd_mstep(SRC, fixed, ONES6, ONES6, px, False)
                out["mstep"][i], out["t_mstep"][i], out["scale"][i], out["sigma2"][i] = R, t, s, s2
            print("%s form: %d matrices solved on each path" % (form, n))
            cache[form] = out
        return cache[form]
    return get


def differing_classes(cat, mask):
    return {str(k): int(v) for k, v in zip(*np.unique(cat.names[mask], return_counts=True))}


@pytest.mark.parametrize("path", PATHS)
def test_ieee_form_is_the_oracle_bit_for_bit(solved, cat, path):
    R = solved("ieee")[path]
    differ = ~(bits(R) == bits(cat.R_oracle)).all(axis=1)
    assert not differ.any(), "IEEE form differs from the oracle on %s" % differing_classes(cat, differ)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("form", FORMS)
def test_every_matrix_finite_orthogonal_optimal(solved, cat, form, path):
    R = solved(form)[path]
    assert np.isfinite(R).all()
    e, de = orthogonality(R)
    print("%s/%s: max |R^T R - I| %.2e, |det R - 1| %.2e (host form %.2e, %.2e)" % (form, path, e.max(), de.max(), cat.orth_host, cat.det_host))
    assert e.max() <= 4 * cat.orth_host and de.max() <= 4 * cat.det_host, differing_classes(cat, (e > 4 * cat.orth_host) | (de > 4 * cat.det_host))
    # the Kabsch objective: sigma_1 + sigma_2 + d sigma_3 is the maximum of tr(R^T H) over rotations -- attained even where R is not unique
    deficit = objective_deficit(R, cat.H, cat.S64, cat.d)
    assert deficit.max() <= 16 * EPS, differing_classes(cat, deficit > 16 * EPS)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("form", FORMS)
def test_continuous_part_against_float64(solved, cat, form, path):
    # well-posed (eps sigma_1 / g <= 1e-4) and the band up to the guard's threshold (g >= 0.8e-3 sigma_1), where either form may answer
    R = solved(form)[path]
    ratio = np.abs(R.astype(np.float64) - cat.R64).max(axis=(1, 2)) / (cat.cond + EPS)
    worst = int(np.argmax(np.where(~cat.ill, ratio, 0)))
    print("%s/%s vs float64: worst ratio %.3f (%s); well-posed %d, band %d" % (form, path, ratio[worst], cat.names[worst], cat.well.sum(),
                                                                              (~cat.well & ~cat.ill).sum()))
    assert (ratio[~cat.ill] <= 32).all(), differing_classes(cat, ~cat.ill & (ratio > 32))
    check_measured("kabsch3_%s_%s_vs_f64_ratio" % (form, path), ratio[cat.well].max(), 32.0)


@pytest.mark.parametrize("path", PATHS)
def test_discontinuous_part_is_decided_by_the_ieee_form(solved, cat, path):
    # mirror ties (det(U V^T) < 0, sigma_2 ~ sigma_3: the exact reflections, the det < 0 ties up to a 1e-5 gap) and rank deficiency: R jumps
    # under a one-ulp change of H, so rounding differences between the forms would be differences of branch.  There the fast form must
    # hand over to the IEEE one, whose bits are the oracle's.
    fast, ieee = solved("fast")[path], solved("ieee")[path]
    ill = cat.ill
    assert ill.sum() > 700
    differ = ill & ~(bits(fast) == bits(ieee)).all(axis=1)
    print("%s: fast form on %d ill-posed matrices (%s)" % (path, ill.sum(), differing_classes(cat, ill)))
    assert not differ.any(), "fast form left the IEEE form's bits on %s" % differing_classes(cat, differ)
    assert (bits(fast)[ill] == bits(cat.R_oracle)[ill]).all()


@pytest.mark.parametrize("form", FORMS)
def test_both_consumers_agree(solved, cat, form):
    out = solved(form)
    differ = ~(bits(out["kabsch"]) == bits(out["mstep"])).all(axis=1)
    assert not differ.any(), "mi_kabsch and mi_cpd_mstep disagree on %s" % differing_classes(cat, differ)
    # cb = 0 exactly, ca = 0 up to the fp64 rounding of its sum (six terms of mixed magnitude): t = ca is at rounding level of fp64
    tiny = 2.0 ** -40 * np.abs(cat.H).max(axis=(1, 2))
    assert (np.abs(out["t_kabsch"]).max(axis=1) <= tiny).all() and (np.abs(out["t_mstep"]).max(axis=1) <= tiny).all()
    # the M-step's scale and sigma^2 (cpd_kernels.hip, after the solve) against float64 evaluations of the same formulas: P1 = Pt1 = 1,
    # Np = 6, cb = ca = 0, sum p1 |b|^2 = 6, sum pt1 |a|^2 = |H|_F^2 / 2
    u = cat.unscaled
    S, d = cat.S64[u], cat.d[u]
    num = S[:, 0] + S[:, 1] + d * S[:, 2]
    scale64 = num / 6.0
    sub = 0.5 * (cat.H[u].astype(np.float64) ** 2).sum(axis=(1, 2))
    sigma2_64 = np.abs(sub - scale64 * num) / 18.0
    e_scale = np.abs(out["scale"][u] - scale64) / (EPS * S[:, 0])
    tol2 = EPS * (sub + scale64 * num + num * S[:, 0])
    e_sigma2 = np.abs(out["sigma2"][u] - sigma2_64) / tol2
    print("%s M-step: scale within %.2f eps sigma_1, sigma^2 within %.3f of its tolerance" % (form, e_scale.max(), e_sigma2.max()))
    check_measured("kabsch3_%s_mstep_scale_err_eps_sigma1" % form, e_scale.max(), 4.0)
    check_measured("kabsch3_%s_mstep_sigma2_err_rel_tol" % form, e_sigma2.max(), 1.0)


@pytest.mark.parametrize("form", FORMS)
def test_translation_with_offset_clouds(solved, ctx, ieee_ctx, cat, form):
    # dyadic offsets on both clouds: the source stays exact, the target rounds -- the float64 reference is taken from the float32 clouds as passed
    c = ctx if form == "fast" else ieee_ctx
    rng = np.random.default_rng(7)
    pick = np.nonzero(cat.well & np.isin(cat.names, ["gaussian", "rot_diag", "rotation", "tie_det_neg_0.01", "rank2"]))[0]
    pick = rng.permutation(pick)[:400]
    worst_r, worst_t, used = 0.0, 0.0, 0
    for i in pick:
        ob, oa = rng.integers(-32, 33, 3) / 8.0, rng.integers(-32, 33, 3) / 8.0
        src = (SRC + ob).astype(np.float32)
        tgt = (moving_images(cat.H[i]) + oa).astype(np.float32)
        R, t, n = c.kabsch(src, tgt, IDX)
        s64, t64p = src.astype(np.float64), tgt.astype(np.float64)
        cb, ca = s64.mean(axis=0), t64p.mean(axis=0)
        H64 = (t64p - ca).T @ (s64 - cb)
        R64, S64, d64, g64 = kabsch64(H64[None])
        cond, well, _ = posedness(S64, g64)
        if not well[0]:
            continue                                  # (the rounding of the target moved it out of the well-posed part)
        used += 1
        dR = np.abs(R.astype(np.float64) - R64[0]).max()
        worst_r = max(worst_r, dR / (cond[0] + EPS))
        t_ref = ca - R64[0] @ cb
        tol = 3 * np.abs(cb).max() * dR + 8 * EPS * (np.abs(ca).max() + 3 * np.abs(cb).max())
        worst_t = max(worst_t, np.abs(t - t_ref).max() / tol)
    print("%s: %d offset problems, R within %.2f (eps sigma_1 / g + eps), t within %.3f of its bound" % (form, used, worst_r, worst_t))
    assert used >= 300
    assert worst_r <= 32 and worst_t <= 1.0


# ---- the M-step on its own at random shapes, against a float64 restatement of coherentpointdrift.cpp:223-277 and against the oracle
SHAPES = (2, 255, 256, 257, 131072, 131073, 300007)     # both sides of cpd_standalone_sum_blocks' one-block and 512-block limits


def mstep64(b, a, p1, pt1, px, const_scale, scale_in=1.0):
    b, a, px = (np.asarray(x, np.float64) for x in (b, a, px))
    p1, pt1 = np.asarray(p1, np.float64), np.asarray(pt1, np.float64)
    Np = p1.sum()
    cb, ca = (p1 @ b) / Np, (pt1 @ a) / Np
    A = px.T @ b - Np * np.outer(ca, cb)                # (EigenBefore * px)^T - Np centerAfter centerBefore^T
    R, S, d, g = kabsch64(A[None])
    num = S[0, 0] + S[0, 1] + d[0] * S[0, 2]
    sum_a2, sum_b2 = pt1 @ (a * a).sum(axis=1), p1 @ (b * b).sum(axis=1)
    sub = sum_a2 - Np * (ca @ ca)
    den = sum_b2 - Np * (cb @ cb)
    if const_scale:
        scale = scale_in
        sigma2 = abs(sub + den - 2 * num) / (3 * Np)
    else:
        scale = num / den
        sigma2 = abs(sub - scale * num) / (3 * Np)
    t = ca - scale * (R[0] @ cb)
    return dict(R=R[0], S=S[0], d=d[0], g=g[0], A=A, scale=scale, sigma2=sigma2, t=t, Np=Np, cb=cb, ca=ca, num=num, sub=sub, den=den,
                bpx=np.abs(px.T @ b).max(), sum_a2=sum_a2, sum_b2=sum_b2)


@pytest.mark.parametrize("n", SHAPES)
@pytest.mark.parametrize("m", SHAPES)
def test_mstep_random_shapes(ctx, oracle, m, n):
    rng = np.random.default_rng(m * 1000003 + n)
    b = (rng.normal(size=(m, 3)) * 2 + (1.0, -2.0, 0.5)).astype(np.float32)
    a = (rng.normal(size=(n, 3)) * 2 + (0.3, 1.0, -1.0)).astype(np.float32)
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r)) * np.sign(np.linalg.det(q * np.sign(np.diag(r))))
    p1 = rng.uniform(0.05, 1.0, m).astype(np.float32)
    pt1 = rng.uniform(0.05, 1.0, n).astype(np.float32)
    px = (p1[:, None] * (b.astype(np.float64) @ q.T + (0.5, 0.25, -1.0) + rng.normal(scale=0.1, size=(m, 3)))).astype(np.float32)
    for const_scale in (False, True):
        f = mstep64(b, a, p1, pt1, px, const_scale)
        R, t, s, s2 = ctx.cpd_mstep(b, a, p1, pt1, px, const_scale)
        Ro, to, so, s2o = oracle.cpd_mstep(b, a, p1, pt1, px, const_scale)
        assert np.isfinite(R).all() and np.isfinite(t).all() and np.isfinite(s) and np.isfinite(s2)
        # A is formed in fp32 from fp64 sums: entries off by ~eps (|B^T PX| + Np |ca| |cb|), R by that over the gap g
        E = f["bpx"] + f["Np"] * np.abs(f["ca"]).max() * np.abs(f["cb"]).max()
        condA = EPS * E / f["g"] if f["g"] > 0 else np.inf
        dA = 12 * EPS * E                                  # spectral norm of A's rounding (3 x 4 eps per entry)
        dnum = 3 * (dA + 8 * EPS * f["S"][0])
        e, de = orthogonality(R[None])
        assert e[0] <= 64 * EPS and de[0] <= 64 * EPS
        deficit = f["num"] - np.sum(R.astype(np.float64) * f["A"])
        assert deficit <= 16 * EPS * f["S"].sum() + 3 * dA
        if condA <= 1e-4:
            ratio = np.abs(R - f["R"]).max() / (condA + EPS)
            check_measured("mstep_random_R_vs_f64_ratio", ratio, 32.0)
            assert np.abs(Ro - f["R"]).max() <= 32 * (condA + EPS)         # (the oracle is held to the same bound)
            # t = ca - scale R cb
            dscale = 0.0 if const_scale else dnum / f["den"] + abs(f["scale"]) * 8 * EPS * (f["sum_b2"] + f["Np"] * (f["cb"] @ f["cb"])) / f["den"]
            ttol = 2 * (abs(f["scale"]) * 3 * np.abs(f["cb"]).max() * 32 * (condA + EPS) + dscale * 3 * np.abs(f["cb"]).max()
                        + 8 * EPS * (np.abs(f["ca"]).max() + 3 * abs(f["scale"]) * np.abs(f["cb"]).max()))
            assert np.abs(t - f["t"]).max() <= ttol and np.abs(to - f["t"]).max() <= ttol
        else:
            dscale = 0.0 if const_scale else dnum / f["den"] + abs(f["scale"]) * 8 * EPS * (f["sum_b2"] + f["Np"] * (f["cb"] @ f["cb"])) / f["den"]
        # scale and sigma^2: first-order error bounds of their fp32 evaluation, x 2
        if not const_scale:
            assert abs(s - f["scale"]) <= 2 * dscale and abs(so - f["scale"]) <= 2 * dscale, (s, so, f["scale"], dscale)
            dsub = 8 * EPS * (f["sum_a2"] + f["Np"] * (f["ca"] @ f["ca"]))
            s2tol = 2 * (dsub + abs(f["scale"]) * dnum + abs(f["num"]) * dscale + 4 * EPS * abs(f["sub"] - f["scale"] * f["num"])) / (3 * f["Np"])
        else:
            assert s == so == 1.0
            dden = 8 * EPS * (f["sum_b2"] + f["Np"] * (f["cb"] @ f["cb"]))
            dsub = 8 * EPS * (f["sum_a2"] + f["Np"] * (f["ca"] @ f["ca"]))
            s2tol = 2 * (dsub + dden + 2 * dnum + 4 * EPS * (f["sub"] + f["den"] + 2 * abs(f["num"]))) / (3 * f["Np"])
        assert abs(s2 - f["sigma2"]) <= s2tol and abs(s2o - f["sigma2"]) <= s2tol, (s2, s2o, f["sigma2"], s2tol)
        check_measured("mstep_random_sigma2_err_rel_tol", abs(s2 - f["sigma2"]) / s2tol, 1.0)
