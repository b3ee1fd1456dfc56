"""Convergence diagnostics on the GPU: nmc_k_conv's partial sums over the device sample store
(Engine.conv_partials / convergence, samplePosterior(computeDiagnostics=True)).

Reference: tests/convergence_ref.py -- the float64 restatement of the kernel's fixed order,
which the device must match bit for bit, and the bounds for the comparison with the host
route (nestmc.convergence.from_halfchains over Engine.samples(), nmc_variogram's order).
Engines as in test_gpu_waic.py."""

import os

import numpy
import pytest

import convergence_ref as cr
from gpu_cases import synthetic
from nestmc import _lib
from nestmc import convergence as conv
from nestmc.engine import Engine
from oracle import restatement as rs

pytestmark = pytest.mark.gpu

L = 8   # csrc/conv.h NMC_CONV_L: lags per task, and the rows of one unrolled block


def _state(fam, sizes, C, P, pooling, seed=5):
    r = numpy.random.RandomState(seed)
    G = len(sizes)
    value = r.normal(size=(C, P, G)) * 0.3
    if fam.family == "linreg" and P == 3:
        value[:, 2] = 1.0 + numpy.abs(value[:, 2])     # sigma > 0
    lp = numpy.zeros((C, P, G))
    nested = rs.Nested(fam, sizes)
    ll = numpy.array([nested.group_ll(value[c]) for c in range(C)])
    mu = numpy.zeros((C, P)) if pooling == "partial" else None
    s2 = numpy.full((C, P), 0.5) if pooling == "partial" else None
    return value, lp, ll, mu, s2


def _run(fam, sizes, priors, pooling, C, sched=(60, 20, 4), seed=3, sel=None, chain_base=0,
         state=None):
    """An engine after sched[0] iterations on chains sel of the C-chain state."""
    st = state or _state(fam, sizes, C, fam.n_params, pooling)
    sel = numpy.arange(C) if sel is None else numpy.asarray(sel)
    eng = Engine(fam, sizes, len(sel), pooling, priors, seed=seed, chain_base=chain_base)
    pick = lambda a: None if a is None else a[sel]   # noqa: E731
    eng.set_state(*(pick(a) for a in st))
    eng.set_schedule(*sched)
    eng.run(0, sched[0])
    eng.synchronize()
    return eng


def _engine(kind, C, G, N, sched=(60, 20, 4)):
    fam, sizes, priors, pooling, _ = synthetic(kind, C, G, N)
    return _run(fam, sizes, priors, pooling, C, sched)


@pytest.fixture(scope="module")
def eng70(gpu_lib):
    eng = _engine("linreg_partial", 70, 5, 30)
    assert eng.n_rows == 10 and eng.cols == 14
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def eng70_100(gpu_lib):
    eng = _engine("linreg_partial", 70, 5, 30, (120, 20, 1))
    assert eng.n_rows == 100
    yield eng
    eng.close()


def _same(a, b, what):
    a, b = numpy.ascontiguousarray(a), numpy.ascontiguousarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = a.view(numpy.uint64) != b.view(numpy.uint64)
    assert not bad.any(), "%s: %d of %d words differ, first at %s (%r against %r)" % (
        what, bad.sum(), bad.size, numpy.argwhere(bad)[0], a[bad][0], b[bad][0])


def _check_bits(eng, row_begin=0, n_rows=None, n_valid=None):
    vg, mean, m2 = eng.conv_partials(row_begin, n_rows, n_valid)
    n_rows = eng.n_rows - row_begin if n_rows is None else n_rows
    rows = eng.samples()[:, row_begin:row_begin + n_rows]
    rvg, rmean, rm2 = cr.partials(rows, n_valid)
    assert vg.shape == ((eng.C + 63) // 64, eng.cols, n_rows // 2)
    _same(mean, rmean, "mean")
    _same(m2, rm2, "m2")
    _same(vg, rvg, "vg")
    assert numpy.any(vg[:, :, 1:] > 0)
    return vg, mean, m2


# ---- 1. against the restatement, bit for bit ----------------------------------------------
def test_linreg_partial_10_rows(eng70):
    _check_bits(eng70)            # n = 5 < L, the two hyper columns of each parameter included


def test_linreg_partial_100_rows(eng70_100):
    _check_bits(eng70_100)        # n = 50


@pytest.mark.parametrize("kind,C,G,N", [("gauss_none", 65, 4, 25), ("linreg_complete", 3, 1, 200)])
def test_other_families(gpu_lib, kind, C, G, N):
    eng = _engine(kind, C, G, N)
    try:
        _check_bits(eng)
    finally:
        eng.close()


# lag blocks start at lag 1 (t0 = 1 + m L), blocks of L rows: n around L, 2 L and the block
# edges n - 1 = L, 2 L
@pytest.mark.parametrize("n", [2, 3, L - 1, L, L + 1, L + 2, 2 * L - 1, 2 * L, 2 * L + 1,
                               2 * L + 2, 3 * L + 1])
def test_half_lengths_around_a_lag_block(gpu_lib, n):
    eng = _engine("gauss_none", 65, 2, 10, (20 + 2 * n, 20, 1))
    try:
        assert eng.n_rows == 2 * n
        _check_bits(eng)
    finally:
        eng.close()


# ---- 2. window ---------------------------------------------------------------------------------
def test_window(eng70):
    eng = eng70
    vg, _, _ = _check_bits(eng, row_begin=2, n_rows=6)
    assert vg.shape == (2, 14, 3)
    _check_bits(eng, row_begin=6, n_rows=4)              # (the store's last rows)
    for kw in (dict(row_begin=2, n_rows=5), dict(row_begin=0, n_rows=2), dict(n_rows=0),
               dict(row_begin=8, n_rows=4), dict(row_begin=-2, n_rows=4),
               dict(row_begin=0, n_rows=12), dict(n_valid=0), dict(n_valid=71)):
        with pytest.raises(_lib.NestmcError):
            eng.conv_partials(**kw)
    _check_bits(eng)                                     # (the context still works)


# ---- 3. padding chains -------------------------------------------------------------------------
def test_padding(eng70):
    """n_valid = 60 of 70: the 60-chain restatement; the padding chains' mean and m2 entries
    are +0.0 and finish(n_valid=60) does not look at them."""
    eng = eng70
    vg, mean, m2 = _check_bits(eng, n_valid=60)
    assert not vg[1].any() and not mean[:, :, 60:].any() and not m2[:, :, 60:].any()
    rvg, rmean, rm2 = cr.partials(eng.samples()[:60])
    _same(vg[0], rvg[0], "vg of 60 chains")
    _same(mean[:, :, :60], rmean, "mean of 60 chains")
    a = conv.finish(conv.merge(list(vg)), mean, m2, 5, None, n_valid=60)
    poisoned = mean.copy()
    poisoned[:, :, 60:] = numpy.nan
    b = conv.finish(conv.merge(list(vg)), poisoned, m2, 5, None, n_valid=60)
    c = eng.convergence(n_valid=60)
    for k in ("rhat", "effective_n", "mean", "sd"):
        _same(getattr(a, k), getattr(b, k), k)
        _same(getattr(a, k), getattr(c, k), k)
    assert a.m == 120
    _check_bits(eng, n_valid=64)
    _check_bits(eng, n_valid=67)


# ---- 4. shard invariance -----------------------------------------------------------------------
def test_shards_of_whole_chain_blocks_bit_identical(gpu_lib):
    fam, sizes, priors, pooling, _ = synthetic("linreg_partial", 128, 3, 20)
    st = _state(fam, sizes, 128, 2, pooling)
    a = _run(fam, sizes, priors, pooling, 128, state=st)
    b1 = _run(fam, sizes, priors, pooling, 128, state=st, sel=range(0, 64))
    b2 = _run(fam, sizes, priors, pooling, 128, state=st, sel=range(64, 128), chain_base=64)
    try:
        va, ma, qa = a.conv_partials()
        v1, m1, q1 = b1.conv_partials()
        v2, m2_, q2 = b2.conv_partials()
        assert va.shape[0] == 2 and v1.shape[0] == v2.shape[0] == 1
        _same(v1[0], va[0], "block 0")
        _same(v2[0], va[1], "block 1")
        merged = conv.merge(list(v1) + list(v2))
        _same(merged, conv.merge(list(va)), "merged vg")
        ra = a.convergence()
        rb = conv.finish(merged, numpy.concatenate([m1, m2_], 2), numpy.concatenate([q1, q2], 2),
                         5, None)
        for k in ("rhat", "effective_n", "mean", "sd", "V", "T", "converged", "enough_n"):
            _same(getattr(ra, k).astype(numpy.float64), getattr(rb, k).astype(numpy.float64), k)
    finally:
        for e in (a, b1, b2):
            e.close()


# ---- 5. against the host route -----------------------------------------------------------------
def _check_host_route(res, rows, CB, what):
    """res (device route) against from_halfchains of the same rows (numpy's mean / var and
    nmc_variogram): V, rhat, mean, sd within the derived bounds; the same cutoff T on every
    column (the host test shows the routes agree on it) and effective_n within its bound."""
    x = conv.halfchains(rows)
    host = conv.from_halfchains(x)
    tol = cr.tolerances(x, CB)
    worst = {}
    for k in ("V", "rhat", "mean", "sd"):
        err = numpy.abs(getattr(res, k) - getattr(host, k))
        t = numpy.asarray(tol[k], dtype=numpy.float64)
        worst[k] = float(numpy.max(err[t > 0] / t[t > 0])) if numpy.any(t > 0) else 0.0
        print("convergence %s: %s worst err/bound %.3g" % (what, k, worst[k]))
        assert numpy.all(err <= t), (what, k, worst[k])
    assert numpy.array_equal(res.T, host.T), (what, res.T, host.T)
    rel = numpy.abs(res.effective_n - host.effective_n) / numpy.abs(host.effective_n)
    bound = tol["neff_rel"](host.T, host.effective_n)
    print("convergence %s: effective_n worst err/bound %.3g on %d columns"
          % (what, float(numpy.max(rel / bound)), len(rel)))
    assert numpy.all(rel <= bound), (what, rel, bound)
    assert numpy.array_equal(res.converged, host.converged)
    assert numpy.array_equal(res.enough_n, host.enough_n)
    return host


def test_against_host_route(eng70, eng70_100):
    for eng, what in ((eng70, "n = 5"), (eng70_100, "n = 50")):
        res = eng.convergence()
        assert res.m == 140 and res.n == eng.n_rows // 2 and len(res.parameter) == 14
        _check_host_route(res, eng.samples(), 2, what)


# ---- 6. samplePosterior(computeDiagnostics=True) -----------------------------------------------
def _restated_result(rows, header):
    vg, mean, m2 = cr.partials(rows)
    return conv.finish(conv.merge(list(vg)), mean, m2, rows.shape[1] // 2, header)


def _api_case():
    C, G, N = 6, 3, 20
    fam, sizes, priors, pooling, names = synthetic("linreg_partial", C, G, N)
    kw = dict(saveLogLikelihood=False, priorDistribution=priors,
              startingPointValueRange={n: [-0.5, 0.5] for n in names}, displayProgress=False,
              seed=17, return_samples=True, computeDiagnostics=True)
    return (C, 64, 16, names, G, N, pooling, fam), kw       # burn 32, thin 2: 16 rows, n = 8


def test_sample_posterior_compute_diagnostics(gpu_lib, tmp_path):
    from nestmc.sampler import sample_posterior
    args, kw = _api_case()
    mem = sample_posterior(*args, None, **dict(kw, write_files=False))
    res = mem["convergence"]
    assert mem["rows"].shape == (6, 16, 10) and res.parameter == list(mem["header"])
    want = _restated_result(mem["rows"], mem["header"])
    for k in ("rhat", "effective_n", "mean", "sd", "V"):
        _same(getattr(res, k), getattr(want, k), k)
    assert (res.n, res.m) == (8, 12)
    # with files: convergence.csv is write_csv of that result
    out = str(tmp_path / "one")
    one = sample_posterior(*args, out, **dict(kw, write_files=True))
    assert sorted(os.listdir(out)) == ["convergence.csv", "log", "sample"]
    assert numpy.array_equal(one["rows"], mem["rows"])
    assert open(os.path.join(out, "convergence.csv")).read() == conv.csv_text(res)
    assert conv.csv_text(one["convergence"]) == conv.csv_text(res)
    # two engines on one GPU, 3 + 3 chains: other trees, the same formulas
    two = sample_posterior(*args, None, **dict(kw, write_files=False, devices=[0, 0]))
    assert numpy.array_equal(two["rows"], mem["rows"])
    _check_host_route(two["convergence"], mem["rows"], 2, "devices=[0, 0]")
    _check_host_route(res, mem["rows"], 1, "one engine")
    # off by default
    off = sample_posterior(*args, None, **dict(kw, write_files=False, computeDiagnostics=False))
    assert "convergence" not in off


def test_odd_row_count_raises(gpu_lib):
    from nestmc.sampler import record_iterations, sample_posterior, schedule
    args, kw = _api_case()
    assert len(record_iterations(60, *schedule(60, 20))) == 15
    with pytest.raises(ValueError):
        sample_posterior(args[0], 60, 20, *args[3:], None, **dict(kw, write_files=False))
    with pytest.raises(ValueError):                       # two rows: halves of one row
        sample_posterior(args[0], 4, 2, *args[3:], None, **dict(kw, write_files=False))


def test_process_per_device_rank_path(gpu_lib, tmp_path):
    """process_per_device: the rank sends its merged sums and its chains' moments over the host
    group and rank 0 finishes and writes -- with one rank the file and the result are the
    in-process path's bit for bit (the rank-order merge: tests/test_convergence_host.py)."""
    from nestmc.sampler import sample_posterior
    args, kw = _api_case()
    kw = dict(kw, devices=[0])
    one, ppd = str(tmp_path / "one"), str(tmp_path / "ppd")
    r1 = sample_posterior(*args, one, **kw)
    r2 = sample_posterior(*args, ppd, process_per_device=True, **kw)
    assert numpy.array_equal(r1["rows"], r2["rows"])
    for k in ("rhat", "effective_n", "mean", "sd", "V"):
        _same(getattr(r1["convergence"], k), getattr(r2["convergence"], k), k)
    assert open(os.path.join(one, "convergence.csv"), "rb").read() == \
        open(os.path.join(ppd, "convergence.csv"), "rb").read()
