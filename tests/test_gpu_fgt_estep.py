"""GPU suite: the FGT E-step (cpd_fgt.hip: K-centre sweep, model build, Horner evaluation, post kernels) per element against the two
float64 references of tests/fgt_reference.py, on every case of its catalogue and on contexts that change the model build's split, the member
lists and the K-centre sweep.  The bound of each element is u (4 + sqrt(depth)) times the sum of the absolute values of its terms, plus what
the weights carry in (see fgt_reference); the bar on the ratio is R.BAR, fixed before any measurement, and the worst ratio per context and
reference is recorded through check_measured."""
import os

import numpy as np
import pytest

import fgt_reference as R
from conftest import check_measured

pytestmark = pytest.mark.gpu

CONTEXTS = list(R.CONTEXTS)


@pytest.fixture(scope="module")
def cases(oracle):
    return {c.name: c for c in R.catalogue(kcenter=oracle.fgt_kcenter)}


@pytest.fixture(scope="module")
def path_ctx(capi):
    """A context per developer switch (read once, at context creation: as test_gpu_estep.py path_ctx)."""
    made = {}

    def get(name):
        if name not in made:
            sw = R.CONTEXTS[name]
            old = os.environ.get(sw[0]) if sw else None
            if sw:
                os.environ[sw[0]] = sw[1]
            try:
                made[name] = capi.Context(0)
            finally:
                if sw:
                    if old is None:
                        del os.environ[sw[0]]
                    else:
                        os.environ[sw[0]] = old
        return made[name]
    yield get
    for c in made.values():
        c.close()


@pytest.fixture(scope="module")
def refs(cases, oracle):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = R.references(cases[name], kcenter=oracle.fgt_kcenter, ck=oracle.fgt_ck)
        return cache[name]
    return get


@pytest.fixture(scope="module")
def outputs():
    return {}


def run(ctx, c):
    return ctx.cpd_estep_fgt(c.y, c.x, c.weight, c.sigma2, c.sigma2_init, c.e, c.p)


def bits(out):
    p1, pt1, px, L = out
    return [np.asarray(p1).view(np.uint32), np.asarray(pt1).view(np.uint32), np.asarray(px).view(np.uint32), np.float32(L).view(np.uint32)]


@pytest.mark.parametrize("name", [c.name for c in R.catalogue(with_big=True, kcenter=None)] + ["far_members_2x1000_p16", "far_members_2x1000_p12"])
@pytest.mark.parametrize("context", CONTEXTS)
def test_fgt_estep_per_element(path_ctx, cases, refs, outputs, context, name):
    c = cases[name]
    out = run(path_ctx(context), c)
    outputs[context, name] = out
    r = refs(name)
    # NaN exactly where the reference (and with it the oracle, test_fgt_reference.py) has NaN: the empty cells' means; finite elsewhere
    assert not R.nan_mismatch(out, r["A"]), (c, R.nan_mismatch(out, r["A"]))
    for var in ("A", "B"):
        if r[var] is None:
            print("fgt %s %s vs B: not computed (more than %d pairs in reach)" % (context, name, R.B_MAX_PAIRS))
            continue
        res = R.ratios(out, r[var], a=r["A"])
        ratio, q = R.worst(res)
        print("fgt %s %s vs %s: worst %.3f (%s, element %d)%s" % (context, name, var, ratio, q, res[q][1],
                                                                  " [remainder vacuous somewhere]" if r[var]["remainder_vacuous"] else ""))
        check_measured("fgt_estep_%s_vs_%s" % (context, var), ratio, R.BAR)
    # the contexts that change only how the labels and the member lists are made return the default's bits -- where the plan (Z of both
    # sides) is the same; MISLAM_FGT_LISTS_IN_MODEL=0 splits big cells of clouds up to 32 768 points, a different order of the same sums
    if context not in ("default", "splits0"):
        if ("default", name) not in outputs:
            outputs["default", name] = run(path_ctx("default"), c)
        if (R.plan(c, context)["Zy"], R.plan(c, context)["Za"]) == (R.plan(c)["Zy"], R.plan(c)["Za"]):
            got, want = bits(out), bits(outputs["default", name])
            assert all(np.array_equal(u, v) for u, v in zip(got, want)), (context, name)


def test_overflow_case_is_finite(ctx, cases):
    """Members hundreds of sigmas from their cell mean (fgt_reference.far_members): the model build must give the reference's exact 0,
    not 0 * inf = NaN, for every query in reach of those cells."""
    for name in ("far_members_2x1000_p16", "far_members_2x1000_p12"):
        p1, pt1, px, L = run(ctx, cases[name])
        assert np.isfinite(p1).all() and np.isfinite(px).all() and np.isfinite(pt1).all() and np.isfinite(L), name
