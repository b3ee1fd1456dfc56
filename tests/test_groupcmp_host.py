"""nestmc.groupcmp on the host: the numpy route against three nested Python loops, the three
invariants of its docstring, merge, finish on a hand-computed case, the CSV round trip and the
keyword's presence.  Everything is an integer count or an exact function of one: comparisons
are equalities, no tolerances."""

import inspect
import math

import numpy
import pytest

from nestmc import groupcmp as gc


def loops_ref(raw, P, G, partial, n_valid):
    """The definitions as written: per sample and parameter, every ordered pair."""
    rows, cols, C = raw.shape
    pc = 2 if partial else 0
    hist = numpy.zeros((P, G, G), dtype=numpy.int64)
    wins = numpy.zeros((P, G, G), dtype=numpy.int64)
    bad = numpy.zeros(P, dtype=numpy.int64)
    for r in range(rows):
        for c in range(n_valid):
            for p in range(P):
                th = [float(raw[r, p * (G + pc) + pc + g, c]) for g in range(G)]
                for g in range(G):
                    if math.isnan(th[g]) or math.isinf(th[g]):
                        bad[p] += 1
                    rank = 0
                    for h in range(G):
                        if th[h] < th[g]:
                            rank += 1
                        if th[g] > th[h]:
                            wins[p, g, h] += 1
                    hist[p, g, rank] += 1
    return dict(hist=hist, wins=wins, nonfinite=bad, n_samples=rows * n_valid)


def same(a, b):
    for k in ("hist", "wins", "nonfinite"):
        assert numpy.array_equal(a[k], b[k]), k
    assert a["n_samples"] == b["n_samples"]


def store(seed, rows, P, G, partial, C, kind="normal"):
    r = numpy.random.RandomState(seed)
    cols = P * (G + (2 if partial else 0))
    if kind == "normal":
        return r.normal(size=(rows, cols, C))
    # few distinct values: many exact ties, and zeros of both signs
    x = r.randint(-2, 3, size=(rows, cols, C)).astype(numpy.float64)
    return numpy.where(r.uniform(size=x.shape) < 0.5, x, -x)


def check_invariants(raw, counts, P, G, partial, n_valid):
    S = counts["n_samples"]
    H, W = counts["hist"], counts["wins"]
    assert numpy.all(H.sum(axis=2) == S)
    assert numpy.array_equal(W.sum(axis=2), (H * numpy.arange(G)).sum(axis=2))
    col = gc.group_columns(P, G, partial)
    for p in range(P):
        th = raw[:, col[p], :n_valid]
        with numpy.errstate(invalid="ignore"):
            a, b = th[:, :, None, :], th[:, None, :, :]
            eq = (~(a < b) & ~(a > b)).sum(axis=(0, 3))    # equal, or unordered (a NaN)
        assert numpy.array_equal(W[p] + W[p].T, S - eq)
        assert not W[p].diagonal().any()


@pytest.mark.parametrize("partial", [False, True])
@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("kind", ["normal", "ties"])
def test_counts_against_loops(partial, P, kind):
    G, rows, C, n_valid = 5, 3, 4, 3
    raw = store(11 + P, rows, P, G, partial, C, kind)
    raw[:, :, n_valid:] = numpy.nan                # padding chains: never read
    if partial:                                    # the hyper columns are no groups
        raw[:, 0, :] = 1e300
        raw[:, 1, :] = -1e300
    got = gc.counts_from_samples(raw, P, G, partial, n_valid)
    same(got, loops_ref(raw, P, G, partial, n_valid))
    assert not got["nonfinite"].any()
    assert got["hist"].dtype == got["wins"].dtype == numpy.int64
    check_invariants(raw, got, P, G, partial, n_valid)
    if kind == "ties":
        assert (got["wins"] + numpy.transpose(got["wins"], (0, 2, 1))
                < got["n_samples"]).any(), "the case holds no tie"


def test_signed_zeros_and_all_equal():
    raw = numpy.zeros((2, 4, 3))
    raw[:, 1] = -0.0
    raw[1, 2] = -0.0
    got = gc.counts_from_samples(raw, 1, 4, False)
    assert got["n_samples"] == 6
    assert numpy.all(got["hist"][:, :, 0] == 6) and not got["hist"][:, :, 1:].any()
    assert not got["wins"].any() and not got["nonfinite"].any()
    same(got, loops_ref(raw, 1, 4, False, 3))


def test_nan_and_inf():
    raw = store(5, 2, 2, 4, True, 3)
    col = gc.group_columns(2, 4, True)
    raw[0, col[0, 1], 0] = numpy.nan
    raw[1, col[0, 2], 2] = numpy.inf
    raw[1, col[1, 0], 1] = -numpy.inf
    raw[0, col[1, 3], 1] = numpy.nan
    raw[0, col[1, 2], 1] = numpy.nan
    got = gc.counts_from_samples(raw, 2, 4, True)
    assert list(got["nonfinite"]) == [2, 3]
    same(got, loops_ref(raw, 2, 4, True, 3))
    # a NaN loses and wins nothing: rank 0, and nobody ranks above for it
    assert numpy.all(got["hist"].sum(axis=2) == 6)
    check_invariants(raw, got, 2, 4, True, 3)


def test_bad_shapes_raise():
    raw = numpy.zeros((2, 6, 3))
    for args in ((1, 1, False), (1, 5, False), (2, 3, True)):
        with pytest.raises(ValueError):
            gc.counts_from_samples(raw, *args)
    for nv in (0, 4):
        with pytest.raises(ValueError):
            gc.counts_from_samples(raw, 1, 6, False, nv)


def test_merge_of_a_chain_split():
    raw = store(7, 4, 2, 6, True, 9, "ties")
    whole = gc.counts_from_samples(raw, 2, 6, True)
    parts = [gc.counts_from_samples(numpy.ascontiguousarray(raw[:, :, a:b]), 2, 6, True)
             for a, b in ((0, 4), (4, 5), (5, 9))]
    same(gc.merge(parts), whole)
    same(gc.merge(parts + [gc.zero_counts(2, 6)]), whole)
    rows = [gc.counts_from_samples(raw[a:b], 2, 6, True) for a, b in ((0, 1), (1, 4))]
    same(gc.merge(rows), whole)
    same(gc.unpack(gc.pack(whole), 2, 6), whole)
    assert gc.merge(parts)["hist"].dtype == numpy.int64
    with pytest.raises(ValueError):
        gc.merge([])


def hand_case():
    # G = 3, S = 4 (rows 2 x chains 2), one parameter, no hyper columns; samples (g0, g1, g2):
    #   (1, 2, 3)  (1, 3, 2)  (2, 1, 3)  (1, 1, 2)
    s = numpy.array([[1, 2, 3], [1, 3, 2], [2, 1, 3], [1, 1, 2]], dtype=numpy.float64)
    return numpy.ascontiguousarray(s.reshape(2, 2, 3).transpose(0, 2, 1))   # [row][g][chain]


def test_finish_hand_case():
    c = gc.counts_from_samples(hand_case(), 1, 3, False)
    # 0-based ranks per sample: (0,1,2) (0,2,1) (1,0,2) (0,0,2)
    assert c["hist"][0].tolist() == [[3, 1, 0], [2, 1, 1], [0, 1, 3]]
    assert c["wins"][0].tolist() == [[0, 1, 0], [2, 0, 1], [4, 3, 0]]
    r = gc.finish(c["hist"], c["wins"], c["n_samples"], ["slope"])
    assert r.n_samples == 4 and r.n_groups == 3 and r.names == ["slope"]
    assert r.mean_rank[0].tolist() == [1.25, 1.75, 2.75]
    # cumulative counts (3,4,4) (2,3,4) (0,1,4) against ceil(0.5 S) = 2, ceil(0.025 S) = 1,
    # ceil(0.975 S) = 4
    assert r.median_rank[0].tolist() == [1, 1, 3]
    assert r.rank_lo[0].tolist() == [1, 1, 2]
    assert r.rank_hi[0].tolist() == [2, 3, 3]
    assert r.p_lowest[0].tolist() == [0.75, 0.5, 0.0]
    assert r.p_highest[0].tolist() == [0.0, 0.25, 0.75]
    assert r.probability_greater(0, 2, 0) == 1.0
    assert r.probability_greater("slope", 1, 0) == 0.5
    assert r.probability_greater("slope", 0, 1) == 0.25
    assert r.ranking("slope").tolist() == [0, 1, 2]
    with pytest.raises(ValueError):
        gc.finish(c["hist"], c["wins"], 5)
    with pytest.raises(ValueError):
        gc.finish(c["hist"], c["wins"], 4, ["a", "b"])


@pytest.mark.parametrize("S", [1, 2, 39, 40, 41, 79, 80, 81, 1000, 204800])
def test_quantile_thresholds_are_the_ceilings(S):
    from fractions import Fraction
    assert (S + 1) // 2 == math.ceil(Fraction(1, 2) * S)
    assert (S + 39) // 40 == math.ceil(Fraction(25, 1000) * S)
    assert (39 * S + 39) // 40 == math.ceil(Fraction(975, 1000) * S)


def test_csv_round_trip(tmp_path):
    raw = store(3, 5, 2, 4, True, 7)
    c = gc.counts_from_samples(raw, 2, 4, True, 6)
    r = gc.finish(c["hist"], c["wins"], c["n_samples"], ["a", "b"])
    gc.write_csvs(r, str(tmp_path))
    rk = open(str(tmp_path / gc.FILE_RANKING)).read().splitlines()
    pw = open(str(tmp_path / gc.FILE_PAIRWISE)).read().splitlines()
    assert rk[0] == "parameter,group,mean_rank,median_rank,rank_lo,rank_hi,p_lowest,p_highest"
    assert pw[0] == "parameter,group,other,wins,p_greater"
    assert len(rk) == 1 + 2 * 4 and len(pw) == 1 + 2 * 4 * 3
    assert rk[1].split(",")[:2] == ["a", "0"] and pw[1].split(",")[:3] == ["a", "0", "1"]
    back = gc.read_csvs(str(tmp_path))
    assert back["names"] == ["a", "b"]
    for k in ("mean_rank", "median_rank", "rank_lo", "rank_hi", "p_lowest", "p_highest", "wins",
              "p_greater"):
        assert numpy.array_equal(back[k], getattr(r, k)), k


def test_keyword_in_both_signatures():
    import posteriorSampling
    from nestmc import sampler
    for f in (posteriorSampling.samplePosterior, sampler.sample_posterior):
        p = inspect.signature(f).parameters["computeGroupComparison"]
        assert p.default is False


def test_complete_pooling_raises_before_anything(tmp_path):
    """One group: ValueError before the family is looked at or a directory made."""
    from nestmc import LinearRegression
    from nestmc.sampler import sample_posterior
    x = numpy.arange(8.0)
    fam = LinearRegression.simple(x, 2.0 * x, sigma=1.0)
    out = str(tmp_path / "never")
    with pytest.raises(ValueError, match="computeGroupComparison"):
        sample_posterior(2, 10, 5, ("a", "b"), 2, 4, "complete", fam, out,
                         priorDistribution=None, computeGroupComparison=True)
    import os
    assert not os.path.exists(out)
