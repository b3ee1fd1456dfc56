"""CPU: tests/prior_ref.py held to account -- the grid holds what it claims, and scipy's own
float64 logpdf, measured against the mpmath reference, has the worst figures that
prior_ref.SCIPY_WORST records (the device's tolerance is 4 times them, so they may not drift)."""

import numpy

import prior_ref as pr


def test_grid_holds_the_edges():
    assert len(pr.combos()) == 5 * (6 + 5 + 3 + 2)
    t = pr.y_targets()
    assert len(t) == 311 and numpy.sum((t > 1e-12) & (t < 1e3)) >= 300
    exact_one = 0
    for loc, scale in pr.LOC_SCALE:
        for at in (0.0, 1.0):
            e = pr.edge_x(loc, scale, at)
            assert e[0] < e[1] < e[2]
            y = (e - loc) / scale
            assert y[0] < y[1] < y[2] and y[0] < at < y[2] and abs(y[1] - at) < 1e-12
            if at == 0.0:
                assert y[1] == 0.0 and e[1] == loc
            exact_one += int(at == 1.0 and y[1] == 1.0 and loc != 0)
        x = pr.grid_x("laplace", loc, scale)
        y = (x - loc) / scale
        assert numpy.sum((numpy.abs(y) > 700) & (numpy.abs(y) < 745.2)) >= 20
        assert numpy.sum(numpy.abs(y) >= 746) >= 8
    assert exact_one >= 2            # y lands exactly on 1 with loc != 0 at (-1, 2) and (100, 10)


def test_scipy_against_the_reference_has_the_recorded_figures():
    worst = dict.fromkeys(pr.FAMILIES, 0.0)
    for c in pr.combos():
        sp = pr.scipy_logpdf(*c)
        pr.check_classification(sp, *c)
        worst[c[0]] = max(worst[c[0]], pr.check_finite(sp, *c))
    print("scipy logpdf against mpmath, worst units per family:",
          {k: round(v, 3) for k, v in worst.items()})
    for name in pr.FAMILIES:
        assert worst[name] <= pr.SCIPY_WORST[name], (name, worst[name])
        assert worst[name] > pr.SCIPY_WORST[name] - 0.011, (name, worst[name])


def test_parent_formula_for_cauchy_is_what_scipy_left_behind():
    """-log(pi) - log1p(y^2) is -inf once y^2 overflows; scipy's two-branch form is not."""
    d = pr.frozen("cauchy", 1.0, 2.0)
    assert abs(d.logpdf(1e155) - -714.2529615334436) < 1e-12
    with numpy.errstate(over="ignore"):
        y = numpy.float64((1e155 - 1.0) / 2.0)
        assert -numpy.log(numpy.pi) - numpy.log1p(y * y) - numpy.log(2.0) == -numpy.inf
