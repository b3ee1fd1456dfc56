"""GPU: runtime-compiled user families (DeviceLikelihood; csrc/user.hip, csrc/fam_user.h) on
every row path, row width and Gibbs mode their step kernel can reach.

user.hip compiles each of its 18 kernels with hiprtc on first use and launches it through
hipModuleLaunchKernel with a hand-written argument array -- nothing the built-in families'
tests exercise.  Every test here asserts from Engine.launch_config() the kernel instance
(nmc_k_run<FamUser, mode, rows>), the row split and the persistence its shape was chosen
for, against rowpath_cases' restatement of choose_geometry (user_step_kernel,
user_gibbs_mode), so a case that stops reaching its path fails.

1. test_user_logistic_on_builtin_paths: a user function with FamLogistic's own expression on
   the logistic cases of the row-path matrix (widths 1..9, the scalar-load and the staged
   loop, the row split) and on two partial-pooling cases beyond LDS: eval_group_ll, flags,
   proposal LLs, recorded rows and the final state BIT FOR BIT the built-in family's, the
   final LLs bit for bit eval_group_ll of the stored values, and the variants of a path
   (NMC_ROWS=bcast, NMC_HALF=0, NMC_PERSIST=0) bit-identical among themselves.
2. test_wide_rows / test_coef16_rows: rows of 10..64 fields (user_models.wide_source; two
   parameters, up to 63 constants) and the 16-parameter model, rows in LDS at the row-block
   edges and rows staged with group starts and ends on odd double offsets: eval_group_ll
   against the numpy.longdouble reference within rowpath_cases.tolerance, the step kernel's
   LLs bit for bit the group kernel's, eval_obs_ll against the per-row reference within
   (48 + 4 (nf + 4)) 2^-53 A_row, chains 0, 1 and C - 1 against the oracle.
3. test_user_gibbs_modes: the Gibbs hand-offs beside the register one (64 groups: its last)
   that a user family never ran -- the payload in LDS (65 .. 96 groups of four parameters), nmc_k_run's all-wave update within one numpy leaf
   (100, 128: the payload of four parameters no longer fits) and over two and five leaves
   (129, 513: a user family never takes nmc_k_sweep) -- persistent and launched per
   iteration, bit-identical to the built-in family on nmc_k_run, every chain against the
   oracle.
4. test_partial_pooling_parameter_limit, test_user_family_compile_limits,
   test_engine_refuses_other_width: the documented limits.  Under partial pooling the
   workgroup state of (14 + nleaf (9 + ntail)) P + 29 columns of 512 bytes must fit the CU's
   160 KiB: with 8 groups at most 12 parameters, which run and match the oracle; 13 to 16 are
   refused by nmc_create (choose_kernel's message) before anything is launched.

What the matrix found: nmc_create refused every table of more than 9 fields ("n_fields must
be 1..9", the built-in families' limit) although nmc_user_family_compile accepts and compiles
families of up to 64 -- no user model of 10..64 fields could be created.  The check now
admits the width a user family was compiled for.

Device error, worst |dev - ref| / (2^-53 A) over 65 + 1 chains per shape, measured on an
MI355X (bound: n_member / 64 + 48 + 4 (nf + 4) for a group, 48 + 4 (nf + 4) for a row):

    model, fields     group, rows in LDS   group, rows staged   row (eval_obs_ll)
    wide, 10          0.74 of 104.6        1.70 of 116.8        3.01 of 104
    wide, 11          1.76 of 108.6        1.68 of 119.6        2.96 of 108
    wide, 16          0.29 of 128.6        2.28 of 136.0        3.19 of 128
    wide, 17          0.50 of 132.6        0.48 of 139.5        3.66 of 132
    wide, 32          0.68 of 192.6        0.97 of 196.0        2.60 of 192
    wide, 33          1.02 of 196.6        0.35 of 199.9        2.35 of 196
    wide, 63          0.80 of 316.6        0.62 of 318.0        1.95 of 316
    wide, 64          0.82 of 320.6        0.97 of 322.0        2.33 of 320
    16 parameters, 16 0.48 of 128.6        0.50 of 132.1        2.11 of 128

The logistic user function has the built-in family's error, being bit-identical to it
(tests/test_gpu_rowpaths.py: 5.56 in LDS, 8.27 staged).
"""

import ctypes
import os

import numpy
import pytest

import rowpath_cases as rp
import user_models
from gpu_cases import run_engine
from nestmc import _lib
from nestmc.engine import Engine
from nestmc.families import DeviceLikelihood, Logistic
from oracle import restatement as rs

pytestmark = pytest.mark.gpu

C = rp.USER_C


def _engine(fam, case, n_chains, env=None, seed=0, chain_base=0):
    with rp.environ(env):
        return Engine(fam, case.sizes, n_chains, case.pooling, rp.model(case.name).priors,
                      seed=seed, chain_base=chain_base)


def _assert_user_path(case, cfg, n_chains, env=None):
    """The launch took the user-family instance the case means to test."""
    kernel, persistent = rp.user_step_kernel(case, n_chains, env)
    what = (case.name, env, cfg)
    assert cfg["kernel"] == kernel, what
    assert cfg["mode"] == kernel.split(", ")[1], what
    assert cfg["split_members"] == case.S, what
    assert cfg["persistent"] == persistent, what
    assert cfg["chains_per_block"] == (32 if "MODE_HALF" in kernel else 64), what


class _Step:
    pass


def _step_run(fam, case, env=None, seed=31, obs_ll=False):
    """A short run (burn 0, thin 1, trace on) from a start whose LLs are the device's own
    eval_group_ll: flags, proposal LLs, rows, launch config, final state, the group kernel's
    LLs of the final values (and eval_obs_ll at them)."""
    value, lp, mu, s2, scale = rp.start(case.name, C)
    n_iter = case.step_iters
    eng = _engine(fam, case, C, env=env, seed=seed, chain_base=3)
    r = _Step()
    r.ll0 = eng.eval_group_ll(value)
    eng.set_state(value, lp, r.ll0, mu, s2, scale=scale)
    eng.set_schedule(n_iter, 0, 1, tune_interval=100)
    eng.set_trace(True)
    eng.run(0, n_iter)
    eng.synchronize()
    r.acc, r.llp = eng.trace(n_iter)
    r.rows = eng.samples()
    r.cfg = eng.launch_config()
    r.state = eng.get_state()
    r.ll1 = eng.eval_group_ll(r.state["value"])
    r.obs = eng.eval_obs_ll() if obs_ll else None
    eng.close()
    return r


def _assert_moves(case, r):
    """Not vacuous: the chains move, in most cells that have rows."""
    nonempty = numpy.asarray(case.sizes) > 0
    moved = r.acc.astype(bool).any(axis=(1, 2))[:, nonempty].mean()
    print("STEP %-26s acceptance %.3f, cells moved %.3f" % (case.name, r.acc.mean(), moved))
    assert moved >= 0.5, (case.name, moved)
    assert 0.05 < r.acc.mean() < 0.95, (case.name, r.acc.mean())
    assert numpy.all(numpy.isfinite(r.ll0))


def _assert_stored_ll(case, r):
    """The step kernel's stored LL is the group kernel's LL of the stored values, and the
    recorded rows of the last iteration are the stored values."""
    bad = numpy.argwhere(r.state["ll"] != r.ll1)
    assert bad.size == 0, (case.name, bad[:5], r.state["ll"][tuple(bad[0])], r.ll1[tuple(bad[0])])
    st = r.state
    last = rs.State(st["value"], st["log_prior"], st["ll"], st["mu"], st["s2"])
    assert numpy.array_equal(r.rows[:, -1, :], rs.row_values(last, case.pooling == "partial"))


def _variants(case):
    v = {}
    if case.lds and case.nf <= 4:
        v["bcast"] = {"NMC_ROWS": "bcast"}            # the one-chain broadcast loop
    if rp.want_half(case, C):
        v["full"] = {"NMC_HALF": "0"}                 # 64 chains per workgroup: NOPOOL
    if case.pooling == "partial" and case.S == 1:
        v["launch"] = {"NMC_PERSIST": "0"}            # one launch per iteration
    return v


# ---------------------------------------------------------------------------------------
# 1. the user logistic on the built-in logistic's cases
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", rp.USER_LOGISTIC + [c.name for c in rp.USER_PARTIAL])
def test_user_logistic_on_builtin_paths(gpu_lib, name):
    case, m = rp.BY_NAME[name], rp.model(name)
    user = user_models.user_logistic(m.fam)
    for n_chains in (C, 1):
        theta = rp.thetas(name, n_chains, seed=n_chains)
        got = []
        for fam in (m.fam, user):
            eng = _engine(fam, case, n_chains)
            if fam is user:
                _assert_user_path(case, eng.launch_config(), n_chains)
            got.append(eng.eval_group_ll(theta))
            eng.close()
        assert numpy.all(numpy.isfinite(got[1])), name
        assert numpy.array_equal(got[0], got[1]), (name, n_chains)
        assert numpy.all(got[1][:, numpy.asarray(case.sizes) == 0] == 0.0)
    base = _step_run(m.fam, case)
    assert base.cfg["kernel"].startswith("nmc_k_run<FamLogistic<%d>" % case.nf), base.cfg
    _assert_moves(case, base)
    variants = {"default": None}
    variants.update(_variants(case))
    kernels = set()
    for vname, env in variants.items():
        u = _step_run(user, case, env=env)
        _assert_user_path(case, u.cfg, C, env)
        kernels.add(u.cfg["kernel"])
        _assert_stored_ll(case, u)
        for k in ("acc", "llp", "rows", "ll0", "ll1"):
            assert numpy.array_equal(getattr(u, k), getattr(base, k), equal_nan=True), \
                (name, vname, k)
        hyper = ("mu", "s2") if case.pooling == "partial" else ()
        for k in ("value", "log_prior", "ll", "scale") + hyper:
            assert numpy.array_equal(u.state[k], base.state[k]), (name, vname, k)
    print("KERNELS %-26s %s" % (name, sorted(kernels)))


# ---------------------------------------------------------------------------------------
# 2. rows wider than any built-in family, and sixteen parameters
# ---------------------------------------------------------------------------------------
def _check_wide(case):
    m = rp.model(case.name)
    fam, nf = m.fam, case.nf
    empty = numpy.asarray(case.sizes) == 0
    # eval_group_ll against the longdouble reference
    for n_chains in (C, 1):
        theta = rp.thetas(case.name, n_chains, seed=n_chains)
        eng = _engine(fam, case, n_chains)
        _assert_user_path(case, eng.launch_config(), n_chains)
        got = eng.eval_group_ll(theta)
        eng.close()
        ref, A = rp.reference(fam, case.sizes, theta)
        tol = rp.tolerance(case.n_member, nf, ref, A)
        err = numpy.abs(numpy.asarray(got.astype(rp.LD) - ref, float))
        worst = rp.ratio(got, ref, A).max()
        print("RATIO group %-24s C=%-2d worst %.3f of %.1f" % (
            case.name, n_chains, worst, rp.bound_units(case.n_member, nf)))
        assert numpy.all(numpy.isfinite(got)), case.name
        bad = numpy.argwhere(~(err <= tol))
        assert bad.size == 0, (case.name, n_chains, bad[:5], worst)
        assert numpy.all(got[:, empty] == 0.0), case.name
    # the step kernel's row loop against the group kernel's, bit for bit
    r = _step_run(fam, case, obs_ll=True)
    _assert_user_path(case, r.cfg, C)
    _assert_moves(case, r)
    _assert_stored_ll(case, r)
    # nmc_k_obs_ll<FamUser> against the per-row reference
    ref, A = rp.reference_rows(fam, case.sizes, r.state["value"])
    tol = rp.bound_units(0, nf) * rp.U * numpy.asarray(A, float)
    err = numpy.abs(numpy.asarray(r.obs.astype(rp.LD) - ref, float))
    worst = rp.ratio(r.obs, ref, A).max()
    print("RATIO obs   %-24s C=%-2d worst %.3f of %.1f" % (case.name, C, worst,
                                                          rp.bound_units(0, nf)))
    bad = numpy.argwhere(~(err <= tol))
    assert bad.size == 0, (case.name, bad[:5], worst)
    # chains 0, 1 and C - 1 against the oracle on the same Philox stream
    run = rp.chain_run(case.name, C)
    acc, llp, rows, cfg = run_engine(run.fam, run.sizes, run.state, numpy.arange(C), run.base,
                                     run.n_iter, run.seed, **run.kw)
    _assert_user_path(case, cfg, C)
    oacc, ollp, orows, margin = rp.run_oracle_of(run)
    sel = run.sel
    bad = numpy.argwhere(acc[sel].astype(bool) != oacc)
    assert bad.size == 0, "%s: flag mismatch at %s (min decision margin %g)" % (
        case.name, bad[:5], margin)
    assert numpy.allclose(llp[sel], ollp, rtol=1e-10, atol=1e-9, equal_nan=True), case.name
    assert numpy.allclose(rows[sel], orows, rtol=1e-9, atol=1e-9, equal_nan=True), case.name
    assert acc.mean() > 0.02


@pytest.mark.parametrize("nf", rp.WIDE_WIDTHS)
def test_wide_rows(gpu_lib, nf):
    """One width, one family: rows in LDS at the row-block edges, rows staged with the big
    group last and first."""
    for case in rp.WIDE_CASES[nf]:
        _check_wide(case)


def test_coef16_rows(gpu_lib):
    """The library's parameter maximum, 16, under none pooling (125 columns of state)."""
    for case in rp.COEF_CASES:
        assert case.P == 16
        _check_wide(case)


# ---------------------------------------------------------------------------------------
# 3. Gibbs modes
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("G,n_chains", [(64, 65), (65, 65), (96, 65), (100, 65), (128, 65), (129, 64),
                                        (513, 64)])
def test_user_gibbs_modes(gpu_lib, G, n_chains):
    """64 chains where two chain blocks of workgroups would not be co-resident (129 groups:
    258 workgroups on 256 CUs), so that the persistent all-wave update over two leaves runs;
    the 513 workgroups of five leaves are never co-resident and run launched per iteration."""
    run = rp.gibbs_run(G, n_chains)
    user = user_models.user_logistic(run.fam)
    kernel, modes = rp.user_gibbs_mode(run.fam, run.sizes)
    want = {64: "SYNC_REG", 65: "SYNC_LDS", 96: "SYNC_LDS", 129: "SYNC", 513: "SYNC"}.get(G)
    assert kernel == "nmc_k_run<" and (want is None or modes[0] == "NMC_MODE_" + want), modes
    lds = rp.rows_fit_lds(max(run.sizes), 4, 1, 4, True, G)
    persistent = rp.gibbs_persistent(G, n_chains)
    suffix = ", true>" if lds else ", false>"
    args = (run.sizes, run.state, run.sel, run.base, run.n_iter, run.seed)
    dev = run_engine(user, *args, **run.kw)
    launch = run_engine(user, *args, env={"NMC_PERSIST": "0"}, **run.kw)
    builtin = run_engine(run.fam, *args, env={"NMC_SWEEP": "0"} if G > 128 else None, **run.kw)
    mode = modes[0] if persistent else "NMC_MODE_LAUNCH"
    for o, md, pe in ((dev, mode, persistent), (launch, "NMC_MODE_LAUNCH", False)):
        cfg = o[3]
        assert cfg["kernel"] == "nmc_k_run<FamUser, " + md + suffix, cfg
        assert cfg["mode"] == md and cfg["persistent"] == pe, cfg
        assert cfg["split_members"] == 1 and cfg["chains_per_block"] == 64, cfg
    assert builtin[3]["kernel"] == "nmc_k_run<FamLogistic<4>, " + mode + suffix, builtin[3]
    print("KERNELS gibbs G=%d %s | %s" % (G, dev[3]["kernel"], launch[3]["kernel"]))
    for name, o in (("launch", launch), ("builtin", builtin)):
        for k in range(3):
            assert numpy.array_equal(o[k], dev[k], equal_nan=True), (G, name, k)
    oacc, ollp, orows, margin = rp.run_oracle_of(run)
    bad = numpy.argwhere(dev[0].astype(bool) != oacc)
    assert bad.size == 0, "flag mismatch at %s (min decision margin %g)" % (bad[:5], margin)
    assert numpy.allclose(dev[1], ollp, rtol=1e-10, atol=1e-9, equal_nan=True)
    assert numpy.allclose(dev[2], orows, rtol=1e-9, atol=1e-9, equal_nan=True)
    assert numpy.all(numpy.isfinite(dev[2]))
    assert dev[0].mean() > 0.02


# ---------------------------------------------------------------------------------------
# 4. the documented limits
# ---------------------------------------------------------------------------------------
def test_partial_pooling_parameter_limit(gpu_lib):
    P = rp.max_partial_params(2, 20, 8)
    assert P == 12
    run = rp.param_limit_run(P)
    case = rp.RowCase("p-limit", "poly", 2, run.sizes, "partial", False, 1, P=P)
    assert (case.path.lds, case.path.S) == (False, 1)
    kernel, persistent = rp.user_step_kernel(case, C)
    # (the state leaves neither the rows nor the Gibbs payload buffers room: the all-wave
    # update, rows by the scalar-load loop)
    assert kernel == "nmc_k_run<FamUser, NMC_MODE_SYNC, false>" and persistent
    acc, llp, rows, cfg = run_engine(run.fam, run.sizes, run.state, numpy.arange(C), run.base,
                                     run.n_iter, run.seed, **run.kw)
    assert cfg["kernel"] == kernel and cfg["persistent"] and cfg["split_members"] == 1, cfg
    oacc, ollp, orows, margin = rp.run_oracle_of(run)
    sel = run.sel
    bad = numpy.argwhere(acc[sel].astype(bool) != oacc)
    assert bad.size == 0, "flag mismatch at %s (min decision margin %g)" % (bad[:5], margin)
    assert numpy.allclose(llp[sel], ollp, rtol=1e-10, atol=1e-9, equal_nan=True)
    assert numpy.allclose(rows[sel], orows, rtol=1e-9, atol=1e-9, equal_nan=True)
    assert numpy.all(numpy.isfinite(rows)) and acc.mean() > 0.02
    # one parameter more, and the documented maximum: refused when the engine is created
    for Q in (P + 1, 16):
        more = rp.param_limit_run(Q, 1)
        with pytest.raises(_lib.NestmcError, match="exceeds the 160 KiB LDS"):
            Engine(more.fam, more.sizes, C, "partial", None, seed=1)


@pytest.mark.parametrize("nf,P", [(0, 2), (65, 2), (3, 0), (3, 17)])
def test_user_family_compile_limits(gpu_lib, nf, P):
    inc = os.path.join(os.path.dirname(os.path.abspath(_lib.LIB_PATH)), os.pardir, "csrc")
    fid = ctypes.c_int(7)
    rc = gpu_lib.nmc_user_family_compile(user_models.POISSON.encode(), nf, P, inc.encode(),
                                         ctypes.byref(fid))
    assert rc == -1 and fid.value == -1, (rc, fid.value)
    assert gpu_lib.nmc_last_error().decode() == \
        "user family: need 1 <= n_fields <= 64, 1 <= n_params <= 16"


def test_engine_refuses_other_width(gpu_lib):
    """An observation table or a parameter count other than the compiled family's."""
    x, y = user_models.poisson_data(3, 5)
    rows = user_models.poisson_rows(x, y)
    fam = DeviceLikelihood(rows, user_models.POISSON, 2, consts=[0.1])
    fid = fam.family_id()
    nf, P = ctypes.c_int(), ctypes.c_int()
    assert gpu_lib.nmc_user_family_shape(fid, ctypes.byref(nf), ctypes.byref(P)) == 0
    assert (nf.value, P.value) == (3, 2)
    for obs, n_params in ((rows[:, :2], 2), (numpy.hstack([rows, rows]), 2), (rows, 3)):
        other = DeviceLikelihood(obs, user_models.POISSON, n_params, consts=[0.1])
        other.family_id = lambda: fid
        with pytest.raises(_lib.NestmcError, match="compiled for other n_fields / n_params"):
            Engine(other, [5, 5, 5], 2, "partial", None)
    with pytest.raises(_lib.NestmcError, match="n_fields must be 1..9"):
        Engine(Logistic(numpy.ones((4, 10)), numpy.ones(4)), [2, 2], 2, "partial", None)
