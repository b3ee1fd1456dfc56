"""CPU: the cases, path arithmetic, references and oracle runs of the user-family row-path
tests (tests/test_gpu_user_rowpaths.py).

* every new case takes, by the host's arithmetic restated in rowpath_cases, the path it is
  named for: row block, staged chunk and buffer of rows.h at the widths where they change
  regime, rows in LDS or staged, no row split, and the Gibbs mode by group count;
* the float64 host functions of the wide models (what the oracle evaluates) agree with their
  numpy.longdouble references within the bound of the oracle's own summation order, a
  sequential sum: (n - 1 + 48 + 4 (nf + 4)) 2^-53 A;
* every oracle-compared run accepts between 5 % and 95 % of its proposals and decides none by
  a margin below 1e-7, from the oracle's trace alone.  The device's LL differs from the
  oracle's by less than 1e-10 at these sizes, so a flag mismatch on the GPU is then an error
  and not a tie.
"""

import numpy
import pytest

import rowpath_cases as rp
import user_models

C = 3


def test_stage_arithmetic():
    """rows.h nmc_row_block / nmc_stage_rows / nmc_stage_buf at the regime changes."""
    widths = (5, 9, 10, 11, 16, 17, 32, 33, 63, 64)
    assert [rp.row_block(nf) for nf in widths] == [4, 3, 3, 2, 2, 1, 1, 1, 1, 1]
    assert [rp.stage_rows(nf) for nf in widths] == [24, 12, 12, 10, 6, 7, 3, 3, 2, 1]
    for nf in range(1, 65):
        R, SR, buf = rp.row_block(nf), rp.stage_rows(nf), rp.stage_buf(nf)
        assert R >= 1 and SR >= R and SR % R == 0
        # one 1 KiB DMA per chunk: the chunk and a misaligned start's extra double fit it
        assert buf == 128 and SR * nf + 1 <= buf, nf
    # 63 fields: two rows fill the buffer to the last double
    assert rp.stage_rows(63) * 63 + 2 == 128


def test_user_case_paths():
    staged = {10: 821, 16: 513, 17: 483, 33: 249, 63: 131, 64: 129, 11: 745, 32: 257}
    for nf in rp.WIDE_WIDTHS:
        lds, last, first = rp.WIDE_CASES[nf]
        R = rp.row_block(nf)
        assert lds.sizes == [1, R - 1, R, R + 1, 4 * R + 1, 37, 0]
        assert last.sizes == [0, 1, 3, 13, staged[nf]] and first.sizes == last.sizes[-1:] + last.sizes[:-1]
        assert staged[nf] % 2 == 1 and staged[nf] > rp.max_lds_rows("wide", nf, "none", 5)
    assert {10, 16, 17, 33, 63, 64} <= set(rp.WIDE_WIDTHS)
    for c in rp.USER_CASES:
        p = c.path
        assert (p.lds, p.S) == (c.lds, c.S) == (c.name.endswith("-lds"), 1), (c.name, p)
        kernel, persistent = rp.user_step_kernel(c, rp.USER_C)
        if c.pooling == "none":      # wider than the paired loop: never the half layout
            assert kernel == "nmc_k_run<FamUser, NMC_MODE_NOPOOL, %s>" % (
                "true" if c.lds else "false"), c.name
    assert all(c.P == 16 and c.nf == 16 for c in rp.COEF_CASES)
    # partial pooling beyond LDS: register hand-off or a launch per iteration, rows staged
    for c in rp.USER_PARTIAL:
        assert rp.user_step_kernel(c, rp.USER_C) == (
            "nmc_k_run<FamUser, NMC_MODE_SYNC_REG, false>", True)
        assert rp.user_step_kernel(c, rp.USER_C, {"NMC_PERSIST": "0"}) == (
            "nmc_k_run<FamUser, NMC_MODE_LAUNCH, false>", False)
    # the logistic cases of the matrix: the half layout where the paired loop runs
    for name in rp.USER_LOGISTIC:
        c = rp.BY_NAME[name]
        assert c.kind == "logistic"
        half = c.lds and c.nf <= 4
        want = "HALF" if half else "NOPOOL"
        assert rp.user_step_kernel(c, rp.USER_C)[0] == "nmc_k_run<FamUser, NMC_MODE_%s, %s>" % (
            want, "true" if c.lds else "false"), name
        if half:
            for env in ({"NMC_HALF": "0"}, {"NMC_ROWS": "bcast"}):
                assert "NMC_MODE_NOPOOL" in rp.user_step_kernel(c, rp.USER_C, env)[0]


def test_user_gibbs_modes_by_group_count():
    want = {64: ("SYNC_REG", True, 1), 65: ("SYNC_LDS", True, 1), 96: ("SYNC_LDS", True, 1), 100: ("SYNC", True, 1),
            128: ("SYNC", True, 1), 129: ("SYNC", True, 2), 513: ("SYNC", False, 5)}
    assert set(want) == set(rp.USER_GIBBS_G)
    for G, (mode, lds, leaves) in want.items():
        fam, sizes = rp.gibbs_model("logistic4", G)
        assert 16 <= min(sizes) and max(sizes) <= 32
        kernel, modes = rp.user_gibbs_mode(fam, sizes)
        assert (kernel, modes[0]) == ("nmc_k_run<", "NMC_MODE_" + mode), (G, modes)
        assert rp.rows_fit_lds(max(sizes), 4, 1, 4, True, G) == lds, G
        assert len(rp.pairwise_leaves(G)) == leaves
        # the general restatement agrees with gibbs_mode
        case = rp.RowCase("g", "logistic", 4, sizes, "partial", lds, 1)
        assert rp.user_step_kernel(case, 64)[0] == "nmc_k_run<FamUser, NMC_MODE_%s, %s>" % (
            mode, "true" if lds else "false"), G
    # 97 groups: the first whose four-parameter payload no longer fits
    fam, sizes = rp.gibbs_model("logistic4", 97)
    assert rp.user_gibbs_mode(fam, sizes)[1][0] == "NMC_MODE_SYNC"
    # the built-in family sweeps where the user family cannot
    fam, sizes = rp.gibbs_model("logistic4", 129)
    assert rp.gibbs_mode(fam, sizes)[0] == "nmc_k_sweep<"
    assert [rp.gibbs_persistent(G, n) for G, n in ((128, 65), (129, 65), (129, 64), (513, 64))] \
        == [True, False, True, False]


def test_partial_pooling_parameter_limit_arithmetic():
    """(14 + nleaf (9 + ntail)) P + 29 columns of 512 bytes within 160 KiB."""
    for P in range(1, 17):
        assert rp.carve_columns(1, P, True, 8) == 23 * P + 29
    assert rp.max_partial_params(2, 20, 8) == 12
    assert rp.carve_columns(1, 12, True, 8) * 512 == 156160       # 152.5 KiB
    assert rp.carve_columns(1, 16, True, 8) * 512 == 203264       # 198.5 KiB
    # ntail = 7 (G = 7, 15, ...) and more leaves leave room for fewer
    assert rp.max_partial_params(2, 20, 15) == 9
    assert rp.max_partial_params(2, 20, 129) == 8
    assert rp.max_partial_params(2, 20, 513) == 4
    # none pooling holds sixteen parameters, rows in LDS beside them
    assert rp.carve_columns(1, 16, False, 7) == 125


@pytest.mark.parametrize("case", [c for c in rp.USER_CASES if c.kind in ("wide", "coef")], ids=repr)
def test_host_function_inside_bound(case):
    m = rp.model(case.name)
    th = rp.thetas(case.name, C)
    ref, A = rp.reference(m.fam, case.sizes, th)
    nested = rp.FastNested(m.fam, case.sizes)
    got = numpy.array([nested.group_ll(th[c]) for c in range(C)])
    chain = max(case.sizes) - 1
    tol = rp.tolerance(case.n_member, case.nf, ref, A, chain)
    err = numpy.abs(numpy.asarray(got.astype(rp.LD) - ref, float))
    print("%s: worst host ratio %.3f of %.1f" % (case.name, rp.ratio(got, ref, A).max(),
                                                  rp.bound_units(case.n_member, case.nf, chain)))
    assert numpy.all(numpy.isfinite(got)) and numpy.all(err <= tol), case.name
    assert numpy.all(got[:, numpy.asarray(case.sizes) == 0] == 0.0)
    assert numpy.all(A >= numpy.abs(ref))
    # per row
    rref, rA = rp.reference_rows(m.fam, case.sizes, th)
    rgot = numpy.array([nested.obs_ll(th[c]) for c in range(C)])
    rerr = numpy.abs(numpy.asarray(rgot.astype(rp.LD) - rref, float))
    assert numpy.all(rerr <= rp.bound_units(0, case.nf) * rp.U * numpy.asarray(rA, float))


def test_wide_reference_sees_the_field_order():
    """The weights are distinct: the reference with two of them exchanged, or with the fields
    shifted by one, is far outside the bound."""
    case = rp.BY_NAME["wide17-lds"]
    m = rp.model(case.name)
    th = rp.thetas(case.name, C)
    ref, A = rp.reference(m.fam, case.sizes, th)
    rows = m.fam.obs().copy()
    for perm in ([1, 0] + list(range(2, 16)), list(range(1, 16)) + [0]):
        other = user_models.wide_family(numpy.hstack([rows[:, perm], rows[:, 16:]]))
        ref2, _ = rp.reference(other, case.sizes, th)
        tol = rp.tolerance(case.n_member, case.nf, ref, A)
        full = numpy.asarray(case.sizes) > 0
        assert numpy.all(numpy.abs(numpy.asarray(ref2 - ref, float))[:, full] > 1e6 * tol[:, full])


def _trace_ok(run, what):
    oacc, ollp, orows, margin = rp.run_oracle_of(run)
    print("%s: acceptance %.3f, least margin %.3g" % (what, oacc.mean(), margin))
    assert 0.05 < oacc.mean() < 0.95, (what, oacc.mean())
    assert margin >= 1e-7, (what, margin)
    assert numpy.all(numpy.isfinite(orows)), what


@pytest.mark.parametrize("case", [c for c in rp.USER_CASES if c.kind in ("wide", "coef")], ids=repr)
def test_chain_runs_decide_clearly(case):
    _trace_ok(rp.chain_run(case.name), case.name)


@pytest.mark.parametrize("G,n_chains", [(64, 65), (65, 65), (96, 65), (100, 65), (128, 65), (129, 64),
                                        (513, 64)])
def test_gibbs_runs_decide_clearly(G, n_chains):
    _trace_ok(rp.gibbs_run(G, n_chains), "gibbs G=%d" % G)


def test_parameter_limit_run_decides_clearly():
    _trace_ok(rp.param_limit_run(rp.max_partial_params(2, 20, 8)), "p-limit")
