"""CPU suite of the E-step references (tests/estep_reference.py): the bound model against the oracle (cpu-slam's sequential fp32 order),
the plan coverage of the catalogue's shapes, and a mutation check -- the comparator must reject a reference with one pair left out."""
import numpy as np
import pytest

import estep_reference as R

SMALL_PAIRS = 5e6


@pytest.fixture(scope="module")
def cases(oracle):
    return R.attach_constants(R.catalogue(), oracle.cpd_constant)


def small(cases):
    return [c for c in cases if not c.big and not c.sparse and c.m * c.n <= SMALL_PAIRS]


def test_catalogue_is_seeded_and_float32():
    a, b = R.catalogue(with_big=False), R.catalogue(with_big=False)
    assert [c.name for c in a] == [c.name for c in b]
    for c, d in zip(a, b):
        assert c.y.dtype == c.x.dtype == np.float32
        assert np.array_equal(c.y, d.y) and np.array_equal(c.x, d.x)
        assert np.isfinite(c.y).all() and np.isfinite(c.x).all()


def test_plan_mirror_coverage():
    cov = R.coverage(R.catalogue())
    missing = [k for k in R.REQUIRED_COVERAGE if k not in cov]
    assert not missing, missing
    # the mirror itself, at the shapes the issue quotes (256 CUs)
    assert R.plan(100000, 7)["k_chunks"] == 256 and R.plan(7, 100000)["x_chunks"] == 256
    p = R.plan(49000, 49000)
    assert (p["x_chunks"], p["x_chunk_len"], p["mfma_blocks"]) == (22, 2232, [266, 279])
    p = R.plan(100000, 45000)
    assert (p["x_chunks"], p["x_chunk_len"], p["mfma_blocks"]) == (11, 4096, [505, 512])
    p = R.plan(5, 300)
    assert (p["k_chunks"], p["k_last"]) == (1, 5)


def test_classes_are_what_they_claim(cases):
    by = {c.name: c for c in cases}
    assert (by["planar_319x2047"].y[:, 2] == 0).all() and (by["planar_319x2047"].x[:, 2] == 0).all()
    assert np.array_equal(by["duplicate_511x511"].y, by["duplicate_511x511"].x)
    lat = by["lattice_321x1025"]
    assert np.array_equal(lat.y, np.round(lat.y)) and np.array_equal(lat.x, np.round(lat.x))
    assert {round(c.weight, 7) for c in cases} == {1e-6, 0.3, round(1 - 1e-6, 7)}
    assert all(c.constant > 0 and np.isfinite(c.constant) for c in cases)
    out = R.out_of_reach(by["outliers_2049x1025"], False)
    assert out.sum() == 51
    r = R.references(by["radius_lattice_1000x1000"], ("trunc",))["trunc"]["A"]
    assert r["amb"].max() > 0                          # neighbours on the truncation boundary


@pytest.mark.parametrize("mode", ["exact", "trunc"])
def test_references_agree_with_the_oracle(cases, oracle, mode):
    worst = {"A": (0.0, ""), "B": (0.0, "")}
    for c in small(cases):
        if mode == "exact" and not c.exact:
            continue
        r = R.references(c, (mode,))[mode]
        o = oracle.cpd_estep(c.y, c.x, c.constant, c.sigma2) if mode == "exact" else \
            oracle.cpd_estep_truncated(c.y, c.x, c.constant, c.sigma2, c.truncate)
        for var in ("A", "B"):
            ratio, q = R.worst(R.ratios(o, r[var], "oracle"))
            assert ratio <= R.BAR, (c, var, q, ratio)
            if ratio > worst[var][0]:
                worst[var] = (ratio, "%s %s" % (c.name, q))
        # where the oracle's denominator is c alone, so is the reference's
        if mode == "trunc" or c.cls == "outliers":
            out = R.out_of_reach(c, mode == "trunc")
            assert (o[1][out] == 0).all() and (r["A"]["pt1"][out] == 0).all()
    print("oracle against the references (%s): A %.2f (%s), B %.2f (%s)" % (mode, worst["A"][0], worst["A"][1], worst["B"][0], worst["B"][1]))


# classes where one pair is visible: the exact E-step's largest term of a fixed point in every class; the pair just above the
# truncation threshold (p ~ 1e-3) where the elements it feeds are not sums of hundreds of larger terms
MUTATION_EXACT = ["uniform_5x300", "uniform_320x1024", "blobs_577x1009", "planar_319x2047", "lattice_321x1025", "duplicate_511x511",
                  "offset_767x2047", "outliers_2049x1025", "sigma2_0.004_1023x1025", "sigma2_0.05_1023x1025", "sigma2_5_1023x1025"]
MUTATION_TRUNC = ["uniform_5x300", "uniform_320x1024", "planar_319x2047", "offset_767x2047", "outliers_2049x1025", "sigma2_0.05_1023x1025",
                  "sparse_4159x3135", "moved_3001x2993"]


@pytest.mark.parametrize("mode,name", [("exact", n) for n in MUTATION_EXACT] + [("trunc", n) for n in MUTATION_TRUNC])
def test_comparator_rejects_a_dropped_pair(cases, mode, name):
    c = {c.name: c for c in cases}[name]
    ref = R.references(c, (mode,))[mode]["A"]
    assert R.worst(R.ratios(R.outputs_of(ref), ref, "valu"))[0] <= 1.0       # the reference's own fp32 rounding passes
    pair = R.mutation_pair(c, mode)
    cut = R.references(c, (mode,), drop=pair)[mode]["A"]
    for path in (("valu", "mfma") if mode == "exact" else ("culled", "every_pair")):
        ratio, q = R.worst(R.ratios(R.outputs_of(cut), ref, path))
        print("%s %s %s: pair %s dropped -> %.3g (%s)" % (mode, name, path, pair, ratio, q))
        assert ratio > R.BAR, (name, path, pair, ratio)
