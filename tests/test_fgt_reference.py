"""CPU suite of the FGT E-step references (tests/fgt_reference.py): the bound model against the oracle (and cpu-slam itself where it is
built), the plan coverage of the catalogue's shapes, the mutation check -- the comparator must reject reference A with one member, one
constant, one order, one cell or the float32 inv changed -- and the overflow case the catalogue's far_members class exists for."""
import math

import numpy as np
import pytest

import fgt_reference as R

SMALL_PAIRS = 2e7


@pytest.fixture(scope="module")
def cases(oracle):
    return {c.name: c for c in R.catalogue(with_big=False, kcenter=oracle.fgt_kcenter)}


@pytest.fixture(scope="module")
def refs(cases, oracle):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = R.references(cases[name], kcenter=oracle.fgt_kcenter, ck=oracle.fgt_ck)
        return cache[name]
    return get


def small(cases):
    return [c for c in cases.values() if c.m * c.n <= SMALL_PAIRS]


def test_catalogue_is_seeded_and_float32(oracle):
    a = R.catalogue(with_big=False, kcenter=oracle.fgt_kcenter)
    b = R.catalogue(with_big=False, kcenter=oracle.fgt_kcenter)
    assert [c.name for c in a] == [c.name for c in b] and len(a) >= 25
    for c, d in zip(a, b):
        assert c.y.dtype == c.x.dtype == np.float32
        assert np.array_equal(c.y, d.y) and np.array_equal(c.x, d.x)
        assert np.isfinite(c.y).all() and np.isfinite(c.x).all()


def test_plan_mirror(oracle):
    # the host's rules against the oracle's restatement of the reference (K, ndi) and at shapes worked out by hand
    for m, n, s2, s2i in ((300, 500, 1.0, 10.0), (2, 1000, 1.0, 1.0), (256, 256, 0.2, 1e3), (1000, 1500, 0.05, 5e4), (5000, 7000, 0.37, 3.3)):
        assert R.cluster_count(m, n, s2, s2i) == oracle.cpd_fgt_clusters(m, n, s2, s2i)
        for w in R.WEIGHTS:
            assert R.ndi(s2, w, m, n) == np.float32(oracle.cpd_fgt_ndi(s2, w, m, n))
    assert R.model_splits(40000, 2, 120) == 16 and R.model_splits(120000, 51, 120) == 4 and R.model_splits(30000, 51, 120) == 1
    assert R.side_plan(30000, 2, 286) == (1, "lists") and R.side_plan(30000, 2, 286, "lists0") == (16, "sort")
    assert R.side_plan(40000, 2, 120, "splits0") == (1, "sort")
    assert R.predict_splits(300000, 51) == 1 and R.predict_splits(1000, 51) == 16 and R.predict_splits(63, 2) == 2
    assert [tuple(e) for e in R.exponents(3)] == [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (2, 0, 0), (1, 1, 0), (1, 0, 1), (0, 2, 0),
                                                  (0, 1, 1), (0, 0, 2)]
    for p in (1, 2, 5, 8, 16):
        ex = R.exponents(p)
        assert len(ex) == R.pd_of(p) == oracle.fgt_pd(p) and len({tuple(e) for e in ex}) == len(ex)
        # C_a = 2^|a| / a! (the reference's float32 table agrees with the definition to its rounding)
        want = np.array([2.0 ** e.sum() / np.prod([math.factorial(int(v)) for v in e]) for e in ex])
        assert np.allclose(oracle.fgt_ck(p), want, rtol=4 * R.U * p)


def test_plan_coverage(oracle):
    cov = R.coverage(R.catalogue(kcenter=oracle.fgt_kcenter))
    missing = [k for k in R.REQUIRED_COVERAGE if k not in cov]
    assert not missing, missing
    print("plan coverage:", {k: len(v) for k, v in sorted(cov.items())})


def test_oracle_within_the_bound_of_both_references(cases, refs, oracle):
    worst = {"A": (0.0, ""), "B": (0.0, "")}
    vacuous, no_b = [], []
    for c in small(cases):
        o = oracle.cpd_estep_fgt(c.y, c.x, c.weight, c.sigma2, c.sigma2_init, c.e, c.p)
        r = refs(c.name)
        # A reproduces the oracle's NaN pattern (empty cells: NaN means reached by every query)
        assert not R.nan_mismatch(o, r["A"]), (c, R.nan_mismatch(o, r["A"]))
        for var in ("A", "B"):
            if r[var] is None:
                no_b.append(c.name)
                continue
            res = R.ratios(o, r[var], R.oracle_depth_extra(r[var], c.p), a=r["A"])
            ratio, q = R.worst(res)
            assert ratio <= R.BAR, (c, var, q, ratio, res)
            if ratio > worst[var][0]:
                worst[var] = (ratio, "%s %s element %d" % (c.name, q, res[q][1]))
            if var == "B" and r[var]["remainder_vacuous"]:
                vacuous.append(c.name)
    print("oracle against the references: A %.3f (%s), B %.3f (%s)" % (worst["A"] + worst["B"]))
    print("B's remainder allowance exceeds the absolute term sum somewhere in:", vacuous, "; B not computed:", no_b)


@pytest.mark.parametrize("name", ["uniform_300x500_p8", "blobs_1500x2000_p11", "lattice_343x512_p8", "duplicate_fixed_200x80_p5",
                                  "clamp_1000x1500_p8", "far_members_2x1000_p16"])
def test_cpu_slam_within_the_bound(cases, refs, ref, name):
    c = cases[name]
    o = ref.cpd_estep_fgt(c.y, c.x, c.weight, c.sigma2, c.sigma2_init, c.e, c.p)
    r = refs(name)
    assert not R.nan_mismatch(o, r["A"]), R.nan_mismatch(o, r["A"])
    ratio, q = R.worst(R.ratios(o, r["A"], R.oracle_depth_extra(r["A"], c.p)))
    print("cpu-slam %s against A: %.3f (%s)" % (name, ratio, q))
    assert ratio <= R.BAR


def test_classes_are_what_they_claim(cases, refs):
    assert (cases["planar_400x600_p5"].y[:, 2] == 0).all() and (cases["planar_400x600_p5"].x[:, 2] == 0).all()
    assert {round(c.weight, 7) for c in cases.values()} == {1e-6, 0.3, round(1 - 1e-6, 7)}
    # empty cells: everything NaN when the moving cloud has them; P1 / PX NaN, Pt1 finite when only the fixed cloud has them
    a = refs("duplicate_moving_30x40_p5")["A"]
    assert np.isnan(a["p1"]).all() and np.isnan(a["pt1"]).all()
    a = refs("duplicate_fixed_200x80_p5")["A"]
    assert np.isnan(a["p1"]).all() and np.isnan(a["px"]).all() and np.isfinite(a["pt1"]).all()
    for name in ("one_per_cell_256x256_p5", "isolated_64x64_p1_e100"):
        c = cases[name]
        assert R.plan(c)["K"] == c.m == c.n


# cases on which each mutation of reference A must be rejected (the ones where it is visible above the bound)
MUTATION_CASES = {
    "drop_member": ["uniform_300x500_p8", "uniform_63x1000_p5", "uniform_64x4097_p3", "uniform_65x129_p2", "uniform_200x300_p1",
                    "blobs_1500x2000_p11", "blobs_700x900_p16", "planar_400x600_p5", "lattice_343x512_p8", "offset_800x1200_p8",
                    "outliers_1000x1000_p8", "sigma2_100_1000x1100_p3_e10", "clamp_1000x1500_p8", "one_per_cell_256x256_p5"],
    "swap_c": ["uniform_300x500_p8", "uniform_63x1000_p5", "uniform_64x4097_p3", "blobs_1500x2000_p11", "blobs_700x900_p16",
               "planar_400x600_p5", "lattice_343x512_p8", "duplicate_fixed_200x80_p5", "offset_800x1200_p8", "sigma2_0.01_1000x1100_p8_e10",
               "sigma2_1_1000x1100_p8_e1", "clamp_1000x1500_p8", "bigcell_2x30000_p11", "bigcell_2x40000_p8"],
    "order_minus_one": ["uniform_300x500_p8", "uniform_64x4097_p3", "uniform_65x129_p2", "blobs_1500x2000_p11", "planar_400x600_p5",
                        "lattice_343x512_p8", "duplicate_fixed_200x80_p5", "sigma2_0.1_1000x1100_p5_e100", "clamp_1000x1500_p8",
                        "bigcell_2x40000_p8"],
    "skip_cell": ["uniform_300x500_p8", "uniform_63x1000_p5", "uniform_65x129_p2", "blobs_1500x2000_p11", "blobs_700x900_p16",
                  "planar_400x600_p5", "duplicate_fixed_200x80_p5", "outliers_1000x1000_p8", "sigma2_1_1000x1100_p8_e1", "clamp_1000x1500_p8",
                  "one_per_cell_256x256_p5", "bigcell_2x30000_p11", "bigcell_2x40000_p8"],
    "h64": ["isolated_64x64_p1_e100"],
}


@pytest.mark.parametrize("kind,name", [(k, n) for k, names in MUTATION_CASES.items() for n in names])
def test_comparator_rejects_a_mutation(cases, oracle, kind, name):
    c = cases[name]
    ref = R.references(c, kcenter=oracle.fgt_kcenter, ck=oracle.fgt_ck, with_b=False)["A"]
    assert R.worst(R.ratios(R.outputs_of(ref), ref))[0] <= 1.0            # the reference's own fp32 rounding passes
    cut = R.references(c, kcenter=oracle.fgt_kcenter, ck=oracle.fgt_ck, with_b=False, **R.mutation(c, kind, oracle.fgt_kcenter))["A"]
    ratio, q = R.worst(R.ratios(R.outputs_of(cut), ref))
    print("%s %s -> %.3g (%s)" % (kind, name, ratio, q))
    assert ratio > R.BAR, (kind, name, ratio, q)


@pytest.mark.parametrize("name", ["far_members_2x1000_p16", "far_members_2x1000_p12"])
def test_overflow_case(cases, refs, oracle, name):
    """Members hundreds of sigmas from their cell mean: d^(p-1) overflows float32 while exp(-|d|^2) == 0.  The reference's recursion
    multiplies the coordinates onto the seed 0 and gets 0; the library's model formula before the fix formed the powers first and got
    0 * inf = NaN, which every query in reach of the cell then read."""
    c = cases[name]
    o = oracle.cpd_estep_fgt(c.y, c.x, c.weight, c.sigma2, c.sigma2_init, c.e, c.p)
    a = refs(name)["A"]
    for q in (o[0], o[1], o[2], a["p1"], a["pt1"], a["px"]):
        assert np.isfinite(q).all()
    _, inv = R.hsigma_inv(c.sigma2)
    _, lab = oracle.fgt_kcenter(c.x, R.plan(c)["K"])
    xc, _ = oracle.fgt_kcenter(c.x, R.plan(c)["K"])
    d, _ = R._offsets(c.x, xc, lab.astype(np.int64), inv)
    assert np.abs(d).max() > np.finfo(np.float32).max ** (1.0 / (c.p - 1))           # d^(p-1) overflows ...
    assert not np.isfinite(R.kernel_form_coefficient(c, oracle.fgt_kcenter, oracle.fgt_ck)).all()     # ... and the powers-first form is NaN
    assert (R.plan(c)["K"], c.m) == (2, 2)
    # the queries reach the far cells
    assert (R._reach(c.y, xc, inv, c.e).sum(axis=1) >= 1).all()
