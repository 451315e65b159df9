"""GPU suite: the exact E-step (K7a / K7b VALU and MFMA, the post kernels) and the truncated one (culled, cpd_trunc.hip, and every-pair)
per element against the two float64 references of tests/estep_reference.py, on every case of its catalogue.  The bound of each element is
the sum of the absolute values of its terms times u (1 + sqrt(depth)) (see estep_reference); the bar on the ratio is R.BAR, fixed before
any measurement, and the worst ratio per path and reference is recorded through check_measured."""
import os

import numpy as np
import pytest

import estep_reference as R
from conftest import check_measured

pytestmark = pytest.mark.gpu

CASES = R.catalogue()
EXACT = [c.name for c in CASES if c.exact]
ALL = [c.name for c in CASES]
SWITCH = {"valu": ("MISLAM_CPD_MFMA", "0"), "mfma": ("MISLAM_CPD_MFMA", "1"), "culled": ("MISLAM_CPD_TRUNC_CULL", "1"),
          "every_pair": ("MISLAM_CPD_TRUNC_CULL", "0")}


@pytest.fixture(scope="module")
def path_ctx(capi):
    """A context per path, created under its developer switch (read once, at context creation: as test_gpu_cpd.py mfma_ctx)."""
    made = {}

    def get(path):
        if path not in made:
            var, val = SWITCH[path]
            old = os.environ.get(var)
            os.environ[var] = val
            try:
                made[path] = capi.Context(0)
            finally:
                if old is None:
                    del os.environ[var]
                else:
                    os.environ[var] = old
        return made[path]
    yield get
    for c in made.values():
        c.close()


@pytest.fixture(scope="module")
def cases(oracle):
    return {c.name: c for c in R.attach_constants(CASES, oracle.cpd_constant)}


@pytest.fixture(scope="module")
def refs(cases):
    """References computed once per case and mode (the 49 000 x 49 000 one takes about a minute)."""
    cache = {}

    def get(name, mode):
        if (name, mode) not in cache:
            c = cases[name]
            modes = ("exact", "trunc") if c.exact else ("trunc",)
            for md, r in R.references(c, modes).items():
                cache[name, md] = r
        return cache[name, mode]
    return get


def run_and_check(ctx, case, ref, path, truncate):
    if truncate:
        out = ctx.cpd_estep_truncated(case.y, case.x, case.constant, case.sigma2, case.truncate)
    else:
        out = ctx.cpd_estep(case.y, case.x, case.constant, case.sigma2)
    p1, pt1, px, L = out
    assert np.isfinite(p1).all() and np.isfinite(pt1).all() and np.isfinite(px).all() and np.isfinite(L), case
    # fixed points with nothing in reach: the denominator is c alone, Pt1 = 1 - c / c = 0 exactly
    far = R.out_of_reach(case, truncate)
    assert (pt1[far] == 0).all(), (case, int(far.sum()), pt1[far].max())
    for var in ("A", "B"):
        res = R.ratios(out, ref[var], path)
        ratio, q = R.worst(res)
        print("estep %s %s vs %s: worst %.3f (%s, element %d)" % (path, case.name, var, ratio, q, res[q][1]))
        check_measured("estep_%s_vs_%s" % (path, var), ratio, R.BAR)


@pytest.mark.parametrize("name", EXACT)
@pytest.mark.parametrize("path", ["valu", "mfma"])
def test_exact_estep_per_element(path_ctx, cases, refs, path, name):
    run_and_check(path_ctx(path), cases[name], refs(name, "exact"), path, False)


@pytest.mark.parametrize("name", ALL)
@pytest.mark.parametrize("path", ["culled", "every_pair"])
def test_truncated_estep_per_element(path_ctx, cases, refs, path, name):
    run_and_check(path_ctx(path), cases[name], refs(name, "trunc"), path, True)


def bits(out):
    p1, pt1, px, L = out
    return [np.asarray(p1).view(np.uint32), np.asarray(pt1).view(np.uint32), np.asarray(px).view(np.uint32), np.float32(L).view(np.uint32)]


def same_bits(a, b):
    return all(np.array_equal(u, v) for u, v in zip(bits(a), bits(b)))


def test_standalone_estep_does_not_inherit_a_registrations_order(capi, cases):
    """mi_cpd_estep / mi_cpd_estep_truncated after a registration on the same context return, bit for bit, what a fresh context returns:
    a registration under MI_ESTEP_CPU_SEQUENTIAL used to leave its summation order in the context's workspace, and the stand-alone exact
    E-step then ran the sequential parity kernels.  (The primitives always run the default order; reaching the sequential kernels per
    element would need an entry point of its own, which is out of scope here.)"""
    c = cases["blobs_577x1009"]
    b, a = cases["uniform_4097x4099"].y[:1500], cases["uniform_4097x4099"].x[:1400]
    with capi.Context(0) as fresh:
        want = fresh.cpd_estep(c.y, c.x, c.constant, c.sigma2)
        want_t = fresh.cpd_estep_truncated(c.y, c.x, c.constant, c.sigma2, c.truncate)
    with capi.Context(0) as used:
        used.cpd_register(b, a, capi.cpd_params(max_iterations=3, estep_mode=capi.ESTEP_CPU_SEQUENTIAL))
        got = used.cpd_estep(c.y, c.x, c.constant, c.sigma2)
        got_t = used.cpd_estep_truncated(c.y, c.x, c.constant, c.sigma2, c.truncate)
        assert same_bits(got, want)
        assert same_bits(got_t, want_t)
        used.cpd_register(b, a, capi.cpd_params(max_iterations=40, approximation=capi.CPD_APPROX_HYBRID))
        assert same_bits(used.cpd_estep_truncated(c.y, c.x, c.constant, c.sigma2, c.truncate), want_t)
        assert same_bits(used.cpd_estep(c.y, c.x, c.constant, c.sigma2), want)
