"""CPU: the extended-precision reference of the row-path tests (rowpath_cases.reference)
and the bound the GPU tests hold the kernels to.

The bound, for one (chain, group) log-likelihood:

    |value - ref| <= (n_member / 64 + 48 + 4 (nf + 4)) 2^-53 A

with ref the numpy.longdouble sum, A the same sum over absolute addends and n_member the
rows of the largest row-split member (rowpath_cases.bound_units has the derivation).  Here
the float64 oracle (oracle.restatement.Nested.group_ll: numpy's per-row formulas, summed
sequentially -- another order than the kernels') must stay inside it at every shape of the
path matrix.

The first term is the kernels' longest addition chain.  The oracle's chain is n - 1
additions, and it fits n_member / 64 only where its rounding errors cancel like a random
walk: the regression and logistic rows, whose addends differ from row to row.  The gauss
family's rows repeat one mean per group (GaussianMean.from_groups, the reference's example),
so every addend of a group is the same number and every rounding error of the sequential
sum has the same sign: the oracle's error grows like its chain (283 units at 2731 rows,
against the kernels' bound of 119 and the device's own 1.8).  That is the oracle's order,
not a fault of either side, so for gauss cases the first term is the oracle's own chain,
n - 1; the kernels are held to n_member / 64 at every case (tests/test_gpu_rowpaths.py).

Worst observed oracle ratio |oracle - ref| / (2^-53 A): regression and logistic 33.7 (case
scalar-linreg2-8192, bound 200; relative to its bound, split-lds: 33.0 of 114.7); gauss
283.2 of 2806 (scalar-gauss3-2731).  The bound is never below 68.
"""

import numpy
import pytest

import rowpath_cases as rp
from oracle import restatement as rs

C = 3


def test_path_arithmetic():
    """The case matrix reaches the paths it names, by the host's arithmetic."""
    for c in rp.CASES:
        p = c.path
        assert (p.lds, p.S) == (c.lds, c.S), (c.name, p)
    assert rp.BY_NAME["tiles"].sizes[-1] == 3456
    assert [rp.row_block(nf) for nf in range(1, 10)] == [16, 8, 5, 4, 4, 4, 4, 4, 3]
    assert rp.BY_NAME["R-gauss-nf8"].sizes == [1, 3, 4, 5, 16, 16, 0]
    assert [len(rp.pairwise_leaves(G)) for G in (128, 129, 512, 513)] == [1, 2, 4, 5]
    # members beyond LDS under the split, and the scalar window of {x, y} rows
    assert rp.BY_NAME["split-scalar"].n_member * 4 * 8 > 65536
    assert rp.BY_NAME["split-staged"].n_member * 8 * 8 > 65536
    assert rp.BY_NAME["split-lds"].n_member == 2731


def test_reference_known_answers():
    """The longdouble formulas against scipy on a tiny table, and A >= |ref|."""
    import scipy.stats
    from nestmc.families import GaussianMean, LinearRegression, Logistic
    r = numpy.random.RandomState(0)
    sizes = [3, 0, 4]
    X = numpy.hstack([numpy.ones((7, 1)), r.normal(size=(7, 2))])
    y = r.normal(size=7)
    fams = [LinearRegression(X, y, sigma=1.3), LinearRegression(X, y),
            Logistic(X, (y > 0).astype(float)), GaussianMean(r.normal(size=(7, 2)), [0.5, 2.0])]
    for fam in fams:
        th = r.normal(size=(2, fam.n_params, 3))
        th[:, -1, :] = numpy.abs(th[:, -1, :]) + 0.1
        ref, A = rp.reference(fam, sizes, th)
        nested = rs.Nested(fam, sizes)
        want = numpy.array([nested.group_ll(th[c]) for c in range(2)])
        assert numpy.allclose(numpy.asarray(ref, float), want, rtol=1e-13, atol=1e-13)
        assert numpy.all(A >= numpy.abs(ref)) and numpy.all(A[:, 1] == 0)


@pytest.mark.parametrize("case", rp.CASES, ids=repr)
def test_oracle_inside_bound(case):
    m = rp.model(case.name)
    th = rp.thetas(case.name, C)
    ref, A = rp.reference(m.fam, case.sizes, th)
    nested = rp.FastNested(m.fam, case.sizes)
    got = numpy.array([nested.group_ll(th[c]) for c in range(C)])
    chain = max(case.sizes) - 1 if case.kind == "gauss" else None
    tol = rp.tolerance(case.n_member, case.nf, ref, A, chain)
    err = numpy.abs(numpy.asarray(got.astype(rp.LD) - ref, float))
    worst = rp.ratio(got, ref, A).max()
    print("%s: worst oracle ratio %.3f of %.1f" % (case.name, worst,
                                                  rp.bound_units(case.n_member, case.nf, chain)))
    assert numpy.all(numpy.isfinite(got))
    assert numpy.all(err <= tol), (case.name, worst)
    empty = numpy.asarray(case.sizes) == 0
    assert numpy.all(got[:, empty] == 0.0)


def test_fast_nested_is_the_oracle():
    """FastNested (arrays instead of lists) returns the oracle's values bit for bit."""
    for name in ("R-logistic-nf5", "R-linreg-nf3", "balance-449", "split-lds"):
        c, m = rp.BY_NAME[name], rp.model(name)
        th = rp.thetas(name, 2)
        slow, fast = rs.Nested(m.fam, c.sizes), rp.FastNested(m.fam, c.sizes)
        for k in range(2):
            assert numpy.array_equal(slow.group_ll(th[k]), fast.group_ll(th[k]))
