"""CPU: the case table of tests/test_gpu_sweep.py (tests/sweep_cases.py).

* paths: every case's predicted path (sweep or not, rows in LDS or not) by the host's
  arithmetic restated in rowpath_cases, the reach table of sweep_cases, and the condition that
  the table reaches all fifteen reachable instantiations of nmc_k_sweep, the sampled-sigma
  forms and the forms without an intercept, in both wave geometries;
* offsets: the parity and placement of the ragged sizes (the prologue's two copy branches);
* nmc_tiles: empty groups, one tile, two, and all sixteen slots;
* oracle trace: every oracle-compared run accepts between 5 % and 95 % of its proposals and
  decides none by a margin below 1e-7, from the oracle's trace alone (the thresholds of
  tests/test_user_rowpath_cases.py); a sampled sigma meets proposals at or below zero.
"""

import numpy
import pytest

import rowpath_cases as rp
import sweep_cases as sc


def test_reach_table():
    for key, want in sc.REACH.items():
        assert tuple(sc.max_rows(*key, G) for G in sc.REACH_G) == want, key
        # (the logistic family has the regression's shape: one accumulator set, P by NF)
        if key[0] == "linreg":
            assert sc.shape("logistic", *key[1:]) == sc.shape(*key)
    # without an intercept a parameter less: more room at the same width
    for nf in (2, 3, 4):
        for G in (129, 256, 512):
            assert sc.max_rows("linreg", nf, False, G) >= sc.max_rows("linreg", nf, True, G)
    # nothing wider fits at any group count the sweep takes, with or without an intercept,
    # sigma known or sampled
    for G in range(129, 513):
        for nf in (7, 8, 9):
            for kind in ("linreg", "linreg_sig", "logistic"):
                for intercept in (True, False):
                    assert sc.max_rows(kind, nf, intercept, G) == 0, (kind, nf, intercept, G)
        assert sc.max_rows("linreg", 6, True, G) == 0 and sc.max_rows("linreg_sig", 5, True, G) == 0
        for nf in range(4, 10):
            assert sc.max_rows("gauss", nf, True, G) == 0, (nf, G)
    for c in sc.CASES:
        if c.role == "unreachable":
            assert (c.kind, c.nf, c.intercept) in sc.UNREACHABLE
            assert not c.sweep and not c.lds and c.kernel.startswith("nmc_k_run<")


def test_case_paths():
    for c in sc.CASES:
        assert c.S == 1 and 128 < c.G <= 512 and len(rp.pairwise_leaves(c.G)) <= 4, c.name
        assert c.sweep == (c.role not in ("over", "unreachable")), c.name
        assert c.lds == c.sweep, c.name
        fam, sizes = sc.model(c.name)
        assert sizes == c.sizes and getattr(fam, "intercept", True) == c.intercept, c.name
        assert (getattr(fam, "sigma", 1.0) is None) == (c.sigma == "sampled"), c.name
        # rowpath_cases.gibbs_mode, the mirror the older sweep tests use, agrees
        assert (rp.gibbs_mode(fam, sizes)[0] == "nmc_k_sweep<") or not c.lds or not c.sweep
        if c.sweep:
            assert c.kernel == "nmc_k_sweep<%s<%d>, NMC_MODE_SYNC_OWN>" % (sc.FAMILY[c.kind], c.nf)
            assert c.waves == (12 if c.C == 64 and c.G <= 136 else 4), c.name
            assert c.resident_batch_fits(), c.name
        assert c.n_iter == (6 if c.G == 512 else 8)
    assert [rp.pairwise_leaves(G) for G in sc.REACH_G] == [[64, 65], [64, 72], [128, 128],
                                                            [128] * 4]


def test_reach_condition():
    """All fifteen instantiations by their exact kernel names, each at C = 65; the forms; one
    case per family at C = 64."""
    by_kernel = {}
    for c in sc.SWEEP_CASES:
        by_kernel.setdefault(c.kernel, []).append(c)
    want = (["FamLinreg<%d>" % nf for nf in range(1, 7)]
            + ["FamLogistic<%d>" % nf for nf in range(1, 7)]
            + ["FamGaussMean<%d>" % nf for nf in range(1, 4)])
    assert sorted(by_kernel) == sorted("nmc_k_sweep<%s, NMC_MODE_SYNC_OWN>" % f for f in want)
    for kernel, cases in by_kernel.items():
        assert any(c.C == 65 and c.waves == 4 and c.role == "ragged" for c in cases), kernel
    forms = {(c.kind, c.nf, c.intercept) for c in sc.SWEEP_CASES if c.role == "ragged"}
    assert {("linreg_sig", nf, True) for nf in (1, 2, 3, 4)} <= forms
    assert {(k, nf, False) for k in ("linreg", "logistic") for nf in (5, 6)} <= forms
    for fam in ("FamLinreg", "FamLogistic", "FamGaussMean"):
        assert any(c.C == 64 and c.waves == 12 and sc.FAMILY[c.kind] == fam
                   for c in sc.SWEEP_CASES), fam
    # each ragged case sits at the smallest of 129 / 136 / 256 groups that holds a row of it
    for c in sc.CASES:
        if c.role == "ragged":
            fits = [G for G in (129, 136, 256) if sc.max_rows(c.kind, c.nf, c.intercept, G) > 0]
            assert c.G == fits[0], c.name
    # at the limit: quad, paired and generic rows, and three accumulator sets; the twin one
    # row beyond leaves LDS
    limits = {c.name: c for c in sc.CASES if c.role == "limit"}
    assert sorted((c.kind, c.nf) for c in limits.values()) == [
        ("gauss", 3), ("linreg", 2), ("linreg", 5), ("logistic", 3)]
    for c in limits.values():
        twin = sc.BY_NAME[c.name.replace("limit-", "over-")]
        big = sc.max_rows(c.kind, c.nf, c.intercept, c.G)
        assert max(c.sizes) == big and sorted(c.sizes)[-2] <= 5, c.name
        assert max(twin.sizes) == big + 1 and not twin.lds and not twin.sweep
        assert [s for s in twin.sizes if s <= 5] == [s for s in c.sizes if s <= 5]
    groups = {(c.kind, c.nf, c.G) for c in sc.CASES if c.role == "groups"}
    assert {(k, nf, G) for k, nf in (("logistic", 3), ("gauss", 2)) for G in sc.REACH_G} <= groups
    for kind, nf in (("logistic", 4), ("gauss", 3), ("linreg", 5)):     # the next wider ones
        assert sc.max_rows(kind, nf, True, 512) == 0
    for name in sc.VARIANT_CASES + [sc.TAKEOVER_CASE, sc.REPLAY_CASE]:
        assert sc.BY_NAME[name].sweep
    assert [(sc.BY_NAME[n].kind, sc.BY_NAME[n].nf, sc.BY_NAME[n].P) for n in sc.VARIANT_CASES] \
        == [("logistic", 4, 4), ("gauss", 3, 3), ("linreg_sig", 2, 3), ("linreg", 3, 3)]


def test_ragged_sizes_and_offsets():
    first_empty = last_empty = 0
    for c in sc.CASES:
        if c.role not in ("ragged", "groups"):
            continue
        R = rp.row_block(c.nf)
        cap = sc.max_rows(c.kind, c.nf, c.intercept, c.G)
        pat = {min(s, cap) for s in (0, 1, R - 1, R, R + 1, 4 * R + 1, 63, 64, 65)}
        assert set(c.sizes) == pat, c.name
        assert any(s % 2 for s in c.sizes) and max(c.sizes) <= cap
        first_empty += c.sizes[0] == 0
        last_empty += c.sizes[-1] == 0
        if c.nf % 2 == 0:
            assert c.sizes[-1] == 0, c.name
            continue
        # odd row width: sweep.h's prologue branches on the parity of the group's first double
        off = c.offsets
        start, nd = off[:-1], numpy.diff(off)
        odd_start = (start % 2 == 1) & (nd > 0)
        even_odd = (start % 2 == 0) & (nd % 2 == 1)
        assert odd_start.sum() >= 10 and even_odd.sum() >= 10, (c.name, odd_start.sum())
        assert (odd_start & (nd % 2 == 1)).any() and (odd_start & (nd % 2 == 0)).any(), c.name
        # the last group: an even start and an odd count of doubles, so the table ends on an
        # odd offset and the DMA's slack double is the first one past the observations
        assert even_odd[-1] and off[-1] % 2 == 1 and c.sizes[-1] > 1, c.name
        assert c.sizes[0] == 0, c.name
    assert first_empty >= 1 and last_empty >= 1
    # NF = 3 and 5 are among the odd widths with that tail, in each family that has them
    tails = {(c.kind, c.nf) for c in sc.CASES if c.role == "ragged" and c.nf % 2 == 1}
    assert {("linreg", 3), ("linreg", 5), ("logistic", 3), ("logistic", 5), ("gauss", 3),
            ("linreg_sig", 3), ("linreg", 1)} <= tails
    # an at-limit group that ends the table (an even count of doubles: no slack), one that
    # starts it, and two in the middle on both start parities
    at = {c.name: c.sizes.index(max(c.sizes)) for c in sc.CASES if c.role == "limit"}
    assert at["limit-logistic3-G129"] == 128 and at["limit-linreg5-G136"] == 0
    c = sc.BY_NAME["limit-gauss3-G129"]
    assert c.offsets[at[c.name]] % 2 == 0 and (max(c.sizes) * c.nf) % 2 == 1


def test_tile_counts():
    """dev.h nmc_tiles: min(16, ceil(n / 64)) tiles of a multiple of 16 rows."""
    assert [len(rp.tiles(n)) for n in (0, 1, 63, 64, 65, 960, 961, 3008)] == [0, 1, 1, 1, 2, 15,
                                                                              16, 16]
    assert rp.tiles(65) == [(0, 48), (48, 17)]
    for c in sc.CASES:
        if c.role in ("ragged", "groups"):
            cap = sc.max_rows(c.kind, c.nf, c.intercept, c.G)
            assert {0, 1} <= set(c.tiles) and (2 in c.tiles) == (cap >= 65), c.name
    nt16 = [c.name for c in sc.SWEEP_CASES if 16 in c.tiles]
    assert "limit-linreg2-G129" in nt16 and "limit-logistic3-G129" in nt16
    # twelve waves: ten queue waves over sixteen tiles; four waves: two over sixteen
    assert sc.BY_NAME["limit-linreg2-G129"].waves == 12
    assert sc.BY_NAME["limit-logistic3-G129"].waves == 4
    assert max(sc.BY_NAME["limit-gauss3-G129"].tiles) == 10


@pytest.mark.parametrize("case", sc.ORACLE_CASES, ids=repr)
def test_oracle_runs_decide_clearly(case):
    assert case.role in ("ragged", "limit") and case.sweep
    oacc, ollp, orows, margin = sc.oracle_of(case.name)
    run = sc.run_of(case.name)
    assert list(run.sel) == [0, 1, case.C - 1] and run.kw["burn"] == 0 and run.kw["thin"] == 1
    assert oacc.shape == (3, case.n_iter, case.P, case.G) and orows.shape[1] == case.n_iter
    print("%s: acceptance %.3f, least margin %.3g" % (case.name, oacc.mean(), margin))
    assert 0.05 < oacc.mean() < 0.95, (case.name, oacc.mean())
    assert margin >= 1e-7, (case.name, margin)
    assert numpy.all(numpy.isfinite(orows)), case.name
    empty = numpy.asarray(case.sizes) == 0
    assert numpy.all(ollp[:, :, :, empty] == 0.0)
    if case.sigma == "sampled":
        # a proposal with sigma <= 0 has a NaN likelihood wherever the group has rows
        nan = int(numpy.isnan(ollp[:, :, -1, :][:, :, ~empty]).sum())
        print("%s: %d proposals with sigma <= 0" % (case.name, nan))
        assert nan > 0, case.name
        assert not numpy.isnan(ollp[:, :, :-1, :]).any()
    else:
        assert numpy.all(numpy.isfinite(ollp)), case.name
