"""nestmc.waic on the host: the formulas, the merge and the files (no GPU).

Tolerances and the longdouble reference: tests/waic_ref.py.
"""

import os

import numpy
import pytest

import waic_ref
from nestmc import waic
from waic_ref import U


def _matrix(S, n, seed):
    """ll[S, n]: per-column level in [-40, 0] and spread factor 0.5, 1 or 30."""
    r = numpy.random.RandomState(seed)
    spread = numpy.array([0.5, 1.0, 30.0])[numpy.arange(n) % 3]
    return -40.0 * r.uniform(size=n) + spread * r.normal(size=(S, n))


def _offsets(n, G, seed=0):
    r = numpy.random.RandomState(seed)
    cuts = numpy.sort(r.randint(0, n + 1, size=G - 1))
    return numpy.concatenate([[0], cuts, [n]]).astype(numpy.int64)


def _tuple(ll):
    """One chain's state over its rows ll[R, n], in float64."""
    m = ll.max(axis=0)
    mean = ll.mean(axis=0)
    return numpy.stack([m, numpy.exp(ll - m).sum(axis=0), numpy.full(ll.shape[1], float(len(ll))),
                        mean, ((ll - mean) ** 2).sum(axis=0)])


@pytest.mark.parametrize("S,n", [(36, 200), (65, 40), (700, 60)])
def test_from_ll_matrix_against_longdouble_reference(S, n):
    ll = _matrix(S, n, seed=S)
    res = waic.from_ll_matrix(ll, _offsets(n, 4))
    waic_ref.check(res, ll, what="from_ll_matrix %dx%d" % (S, n))
    assert res.n_obs == n and res.se_waic == 2 * res.se
    assert res.se == float(numpy.sqrt(n * numpy.var(res.elpd_i, ddof=1)))


def test_ddof_zero_would_miss_the_bound():
    """The bound is tight enough to tell the variance's divisor."""
    ll = _matrix(65, 40, seed=1)
    res = waic.from_ll_matrix(ll, [0, 40])
    res.p_waic_i = numpy.var(ll, axis=0, ddof=0)
    with pytest.raises(AssertionError):
        waic_ref.check(res, ll)


def test_merge_orders_and_identity():
    C, R, n = 13, 7, 50
    ll = _matrix(C * R, n, seed=3).reshape(C, R, n)
    flat = ll.reshape(C * R, n)
    parts = [_tuple(ll[c]) for c in range(C)]
    ident = waic.identity(n)
    off = _offsets(n, 5)
    butterfly = list(parts)
    while len(butterfly) > 1:     # pairs, then pairs of pairs, the odd one carried
        butterfly = [waic.merge(butterfly[i:i + 2]) for i in range(0, len(butterfly), 2)]
    orders = {
        "forward": parts,
        "reverse": parts[::-1],
        "shuffled": [parts[i] for i in numpy.random.RandomState(0).permutation(C)],
        "identities": [ident] + [p for q in parts for p in (q, ident)],
        "tree": butterfly,
    }
    for name, seq in orders.items():
        merged = waic.merge(seq)
        assert numpy.all(merged[2] == C * R)
        waic_ref.check(waic.finish(merged, off), flat, what="merge " + name)
    x = waic.merge(parts[:3])
    for seq in ([x, ident], [ident, x], [ident, x, ident, ident]):
        assert waic.merge(seq).tobytes() == x.tobytes()
    assert waic.merge([ident, ident]).tobytes() == ident.tobytes()
    with pytest.raises(ValueError):
        waic.merge([])
    with pytest.raises(ValueError):
        waic.merge([x, waic.identity(n + 1)])


def test_rank_order_merge_of_fabricated_rank_partials():
    """process_per_device: every rank sends its merged partial as bytes, rank 0 merges in
    rank order; a rank of padding chains only sends the identity."""
    C, R, n = 9, 5, 30
    ll = _matrix(C * R, n, seed=8).reshape(C, R, n)
    ranks = [waic.merge([_tuple(ll[c]) for c in cs]) for cs in ([0, 1, 2, 3], [4, 5, 6], [7, 8])]
    ranks.append(waic.identity(n))
    wire = [numpy.ascontiguousarray(p).tobytes() for p in ranks]
    got = waic.merge_ranks([numpy.frombuffer(b, dtype=numpy.float64).reshape(5, -1) for b in wire])
    assert got.tobytes() == waic.merge(ranks).tobytes()
    assert got.tobytes() == waic.merge(ranks[:3]).tobytes()
    waic_ref.check(waic.finish(got, [0, n]), ll.reshape(C * R, n), what="ranks")


def test_finish_needs_two_samples():
    one = _tuple(_matrix(1, 10, seed=2))
    with pytest.raises(ValueError):
        waic.finish(one, [0, 10])
    with pytest.raises(ValueError):
        waic.finish(waic.identity(10), [0, 10])
    with pytest.raises(ValueError):
        waic.from_ll_matrix(_matrix(1, 10, seed=2), [0, 10])
    waic.finish(waic.merge([one, one]), [0, 10])


def test_group_sums():
    n = 200
    ll = _matrix(36, n, seed=4)
    off = numpy.array([0, 1, 1, 60, 199, 200])          # a one-row and an empty group
    res = waic.from_ll_matrix(ll, off)
    assert res.elpd_g.shape == res.p_waic_g.shape == (5,)
    assert res.elpd_g[1] == 0 and res.elpd_g[0] == res.elpd_i[0]
    assert abs(res.elpd_g.sum() - res.elpd) <= n * U * numpy.abs(res.elpd_i).sum()
    assert abs(res.p_waic_g.sum() - res.p_waic) <= n * U * numpy.abs(res.p_waic_i).sum()
    with pytest.raises(ValueError):
        waic.from_ll_matrix(ll, [0, n - 1])


def test_from_directory(tmp_path):
    C, R = 12, 6                                        # (chain 10 sorts after 9, not after 1)
    sizes = [3, 1, 9, 4]
    n = sum(sizes)
    off = numpy.concatenate([[0], numpy.cumsum(sizes)])
    r = numpy.random.RandomState(5)
    ll = -3.0 * r.uniform(size=n) + r.normal(size=(C, R, n))
    os.makedirs(str(tmp_path / "sample"))
    for c in range(C):
        with open(str(tmp_path / "sample" / ("logLikelihood.%d.csv" % c)), "w") as f:
            for row in ll[c]:
                f.write(",".join("%f" % v for v in row) + "\n")
    (tmp_path / "sample" / "sample.0.csv").write_text("b0\n1.0\n")
    got = waic.from_directory(str(tmp_path), off)
    rounded = numpy.array([[[float("%f" % v) for v in row] for row in ll[c]] for c in range(C)])
    want = waic.from_ll_matrix(rounded.reshape(C * R, n), off)
    for k in ("lppd_i", "p_waic_i", "elpd_i", "elpd_g", "p_waic_g"):
        assert numpy.array_equal(getattr(got, k), getattr(want, k)), k
    assert (got.elpd, got.p_waic, got.waic, got.se, got.n_samples) == \
        (want.elpd, want.p_waic, want.waic, want.se, C * R)
    exact = waic.from_ll_matrix(ll.reshape(C * R, n), off)
    for k in ("lppd_i", "p_waic_i", "elpd_i"):
        assert numpy.max(numpy.abs(getattr(got, k) - getattr(exact, k))) <= 1e-5, k
    with pytest.raises(FileNotFoundError):
        waic.from_directory(str(tmp_path / "sample"), off)


def test_write_csvs_round_trip(tmp_path):
    n = 23
    off = numpy.array([0, 5, 5, 23])
    res = waic.from_ll_matrix(_matrix(40, n, seed=6), off)
    waic.write_csvs(res, str(tmp_path))
    a = (tmp_path / "waic.csv").read_text().splitlines()
    assert a[0] == "waic,se_waic,elpd,se_elpd,p_waic,n_samples,n_obs" and len(a) == 2
    v = numpy.loadtxt(str(tmp_path / "waic.csv"), delimiter=",", skiprows=1)
    assert v.tolist() == [res.waic, res.se_waic, res.elpd, res.se, res.p_waic, 40.0, float(n)]
    b = (tmp_path / "waic_pointwise.csv").read_text().splitlines()
    assert b[0] == "obs,group,lppd,p_waic,elpd" and len(b) == n + 1
    p = numpy.loadtxt(str(tmp_path / "waic_pointwise.csv"), delimiter=",", skiprows=1)
    assert numpy.array_equal(p[:, 0], numpy.arange(n))
    assert numpy.array_equal(p[:, 1], numpy.repeat([0, 1, 2], [5, 0, 18]))
    assert numpy.array_equal(p[:, 2], res.lppd_i)
    assert numpy.array_equal(p[:, 3], res.p_waic_i)
    assert numpy.array_equal(p[:, 4], res.elpd_i)
