"""nestmc.convergence on the host: the restatement of nmc_k_conv (tests/convergence_ref.py)
against the longdouble formulas within the derived bounds, merge / finish / from_halfchains /
write_csv.  No GPU: from_halfchains runs with variogram_host (nmc_variogram's order)."""

import os

import numpy
import pytest

import convergence_ref as cr
from nestmc import convergence as conv


def ar1(K, m, n, seed, phi=0.6):
    """x [K][m][n]: AR(1) half-chains around column-dependent levels."""
    r = numpy.random.RandomState(seed)
    e = r.normal(size=(K, m, n))
    x = numpy.empty((K, m, n))
    x[:, :, 0] = e[:, :, 0]
    for q in range(1, n):
        x[:, :, q] = phi * x[:, :, q - 1] + e[:, :, q]
    return x * (1 + numpy.arange(K))[:, None, None] + 3.0 * numpy.arange(K)[:, None, None]


def rows_of(x):
    """x [K][m][n], half-chains (chain, half) -> rows [C][2n][K]."""
    K, m, n = x.shape
    return numpy.ascontiguousarray(numpy.transpose(x.reshape(K, m // 2, 2 * n), (1, 2, 0)))


def restated(x, names=None):
    vg, mean, m2 = cr.partials(rows_of(x))
    return conv.finish(conv.merge(list(vg)), mean, m2, x.shape[2], names), vg, mean, m2


CASES = [(14, 140, 5, 11), (6, 12, 50, 12)]


@pytest.mark.parametrize("K,m,n,seed", CASES)
def test_restatement_within_bounds_of_longdouble(K, m, n, seed):
    x = ar1(K, m, n, seed)
    assert numpy.array_equal(conv.halfchains(rows_of(x)), x)
    res, vg, mean, m2 = restated(x)
    f = cr.longdouble_formulas(x)
    CB = vg.shape[0]
    means = numpy.transpose(mean, (0, 2, 1)).reshape(K, m)
    M2 = numpy.transpose(m2, (0, 2, 1)).reshape(K, m)
    r_mean = numpy.max(numpy.abs(means - f["mean_j"]) / cr.tol_mean(f["absmean_j"], n))
    r_m2 = numpy.max(numpy.abs(M2 - f["M2_j"]) / cr.tol_m2(f["M2_j"], f["absmean_j"], n))
    tv = cr.tol_v_exact(f["V"], n, CB)
    r_v = numpy.max(numpy.abs(res.V - f["V"])[:, 1:] / tv[:, 1:])
    print("restatement against longdouble, x[%d][%d][%d]: worst err/tol mean %.3g, M2 %.3g, "
          "V %.3g" % (K, m, n, r_mean, r_m2, r_v))
    assert r_mean <= 1 and r_m2 <= 1 and r_v <= 1
    assert numpy.all(res.V[:, 0] == 0)
    tol = cr.tolerances(x, CB)
    for name in ("rhat", "sd", "mean"):
        err = numpy.abs(getattr(res, name) - f[name])
        print("  %s: worst err/tol %.3g" % (name, float(numpy.max(err / tol[name]))))
        assert numpy.all(err <= tol[name]), name


@pytest.mark.parametrize("K,m,n,seed", CASES)
def test_same_cutoff_as_host_route(K, m, n, seed):
    """The condition the GPU comparison of effective_n relies on: both routes cut the
    autocorrelation sum at the same lag T on every column of these inputs."""
    x = ar1(K, m, n, seed)
    res, _, _, _ = restated(x)
    host = conv.from_halfchains(x, variogram=conv.variogram_host)
    assert numpy.array_equal(res.T, host.T)
    tol = cr.tolerances(x, (m // 2 + 63) // 64)
    assert numpy.all(numpy.abs(res.V - host.V) <= tol["V"])
    rel = numpy.abs(res.effective_n - host.effective_n) / numpy.abs(host.effective_n)
    bound = tol["neff_rel"](host.T, host.effective_n)
    print("neff: worst err/bound %.3g" % float(numpy.max(rel / bound)))
    assert numpy.all(rel <= bound)
    assert numpy.array_equal(res.converged, host.converged)
    assert numpy.array_equal(res.enough_n, host.enough_n)


def test_merge_identity_blocks_change_nothing():
    x = ar1(3, 256, 6, 5)
    vg, mean, m2 = cr.partials(rows_of(x))
    assert vg.shape[0] == 2
    z = numpy.zeros_like(vg[0])
    a = conv.merge(list(vg))
    b = conv.merge([z, vg[0], z, vg[1], z])
    assert a.tobytes() == b.tobytes()
    ra = conv.finish(a, mean, m2, 6, None)
    padded = numpy.concatenate([mean, numpy.zeros((3, 2, 7))], axis=2)
    rb = conv.finish(b, padded, numpy.concatenate([m2, numpy.zeros((3, 2, 7))], axis=2), 6, None,
                     n_valid=128)
    for k in ("rhat", "effective_n", "mean", "sd", "V"):
        assert getattr(ra, k).tobytes() == getattr(rb, k).tobytes(), k
    assert ra.m == rb.m == 256


def test_two_parts_merge_to_the_128_chain_bits():
    """Two 64-chain parts (an engine each) against one 128-chain restatement: the chain
    blocks are the same trees, the merge adds them in the same order."""
    x = ar1(4, 256, 7, 9)
    rows = rows_of(x)
    vg, mean, m2 = cr.partials(rows)
    v1, mean1, m21 = cr.partials(rows[:64])
    v2, mean2, m22 = cr.partials(rows[64:])
    assert v1[0].tobytes() == vg[0].tobytes() and v2[0].tobytes() == vg[1].tobytes()
    merged = conv.merge(list(v1) + list(v2))
    assert merged.tobytes() == conv.merge(list(vg)).tobytes()
    a = conv.finish(merged, numpy.concatenate([mean1, mean2], 2),
                    numpy.concatenate([m21, m22], 2), 7, None)
    b = conv.finish(conv.merge(list(vg)), mean, m2, 7, None)
    for k in ("rhat", "effective_n", "mean", "sd", "V", "T"):
        assert getattr(a, k).tobytes() == getattr(b, k).tobytes(), k


def test_rank_merge_order():
    """merge_ranks adds left to right: three blocks whose sum depends on the order."""
    p = [numpy.full((1, 2), v) for v in (1.0, 2.0 ** -53, 2.0 ** -53)]
    assert conv.merge_ranks(p)[0, 0] == 1.0                      # (1 + u) + u, rounded twice
    assert conv.merge_ranks(p[::-1])[0, 0] == 1.0 + 2.0 ** -52   # (u + u) + 1
    assert conv.merge(p).tobytes() == conv.merge_ranks(p).tobytes()
    with pytest.raises(ValueError):
        conv.merge([])
    with pytest.raises(ValueError):
        conv.merge([numpy.zeros((1, 2)), numpy.zeros((2, 2))])


def test_write_csv_text(tmp_path):
    res = conv.ConvergenceResult(["b[001]", "a_mu", "b[000]"], [1.0004, 1.25, 1.09996],
                                 [812.3456, 12.5, 40.0004], [0.5, -2.25, 1e-7],
                                 [1.0, 0.125, 2.0000005], numpy.zeros((3, 4)), [1, 2, 3], 4, 4)
    assert res.converged.tolist() == [True, False, True]
    assert res.enough_n.tolist() == [True, False, True]
    conv.write_csv(res, str(tmp_path))
    text = open(os.path.join(str(tmp_path), "convergence.csv")).read()
    assert text == ("parameter,rhat,converged,effective n,enough n,mean,sd\n"
                    "'a_mu',1.250,False,12.500,False,-2.250000,0.125000\n"
                    "'b[000]',1.100,True,40.000,True,0.000000,2.000001\n"
                    "'b[001]',1.000,True,812.346,True,0.500000,1.000000\n")
    assert text == conv.csv_text(res)


def test_too_short_half_chains_raise():
    with pytest.raises(ValueError):
        conv.finish(numpy.zeros((2, 1)), numpy.zeros((2, 2, 3)), numpy.zeros((2, 2, 3)), 1, None)
    with pytest.raises(ValueError):
        conv.from_halfchains(numpy.zeros((2, 6, 1)), variogram=conv.variogram_host)
    with pytest.raises(ValueError):
        conv.halfchains(numpy.zeros((3, 5, 2)))
    with pytest.raises(ValueError):
        conv.halfchains(numpy.zeros((3, 2, 2)))
