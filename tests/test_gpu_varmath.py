"""GPU: the variate math and the hyper draws on the device, at their edges.

* nmc_log_unit, nmc_cos2pi, nmc_box_muller: the device returns the host's words on every input
  of tests/varmath_ref.py, so tests/test_varmath_host.py's sweep against mpmath stands for the
  device as well.
* nmc_igamci on the device against the mpmath roots (integer and half-integer shapes, the ends
  of the replayed uniform's grid, both sides of the q < 1/2 switch), and its special values.
* The Philox block on counters with 0, 1, 2^31 and 2^32 - 1 in every word.
* nmc_gamma_mt against the oracle draw by draw (boosted and not, second attempts included),
  and as a distribution.
* The recorded hyper rows of a Philox run (nmc_k_fill<false>, the sweep's in-kernel draw) tied
  bit for bit to the stream's specification, G = 2 and 3 included.
"""

import ctypes

import numpy
import pytest
import scipy.special

import gibbs_order as go
import varmath_ref as vr
from nestmc.engine import Engine
from oracle import philox as ph
from oracle import restatement as rs
from rowpath_cases import environ as _environ, gibbs_mode as _gibbs_mode, \
    gibbs_model as _gibbs_model

pytestmark = pytest.mark.gpu


def _rng(lib, ctr, seed, shape):
    """nmc_debug_rng: [n, 4] = {Box-Muller normal, uniform a, uniform b, Gamma(shape) draw}."""
    ctr = numpy.ascontiguousarray(ctr, dtype=numpy.uint32)
    out = numpy.empty((len(ctr), 4))
    rc = lib.nmc_debug_rng(ctr.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), len(ctr),
                           int(seed), float(shape),
                           out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
    assert rc == 0
    return out


@pytest.mark.parametrize("name", ["log_unit", "cos2pi", "box_muller"])
def test_device_words_equal_host_words(gpu_lib, name):
    extra = vr.device_extra()
    if name == "log_unit":
        which, a = vr.WHICH_LOG, numpy.concatenate([vr.log_inputs(), extra])
        b = a
    elif name == "cos2pi":
        u = vr.cos_inputs()
        which = vr.WHICH_COS
        a = numpy.concatenate([u, 1.0 - u, 0.5 - u[u <= 0.5], extra])
        b = a
    else:
        ua, ub = vr.bm_inputs()
        which = vr.WHICH_BM
        a = numpy.concatenate([ua, numpy.repeat(extra, len(extra))])
        b = numpy.concatenate([ub, numpy.tile(extra, len(extra))])
    host = vr.varmath(gpu_lib, which, a, b, 0)
    dev = vr.varmath(gpu_lib, which, a, b, 1)
    bad = vr.same_words(host, dev)
    print("VARMATH device %s: %d inputs, %d words differ from the host's"
          % (name, len(a), bad.size))
    assert bad.size == 0, [(a[i], b[i], host[i], dev[i]) for i in bad[:8]]


def test_device_igamci_against_mpmath_root(gpu_lib):
    a, q = vr.igamci_inputs()
    a, q = numpy.array(a), numpy.array(q)
    lga = numpy.ascontiguousarray(scipy.special.gammaln(a))
    P = lambda v: v.ctypes.data_as(ctypes.POINTER(ctypes.c_double))   # noqa: E731
    dev = numpy.empty_like(a)
    assert gpu_lib.nmc_debug_igamci(P(a), P(q), P(lga), len(a), P(dev)) == 0
    err = vr.igamci_rel(dev, vr.igamci_reference())
    host = vr.igamci_host(gpu_lib, a, q)
    diff = numpy.abs(dev / host - 1.0)
    worst = int(numpy.argmax(err))
    print("VARMATH igamci device: worst %.3e at (a, q) = (%g, %r); device against host: worst "
          "%.3e" % (err[worst], a[worst], q[worst], diff.max()))
    bad = numpy.flatnonzero(~(err <= vr.IGAMCI_RTOL))
    assert bad.size == 0, [(a[i], q[i], dev[i], err[i]) for i in bad[:8]]
    sa = numpy.array([s[0] for s in vr.IGAMCI_SPECIAL])
    sq = numpy.array([s[1] for s in vr.IGAMCI_SPECIAL])
    want = numpy.array([s[2] for s in vr.IGAMCI_SPECIAL])
    with numpy.errstate(all="ignore"):
        sl = numpy.ascontiguousarray(scipy.special.gammaln(sa))
    got = numpy.empty_like(sa)
    assert gpu_lib.nmc_debug_igamci(P(sa), P(sq), P(sl), len(sa), P(got)) == 0
    assert vr.same_words(got, want).size == 0, (got, want)


def test_counter_words_at_their_edges(gpu_lib):
    """Uniforms bit for bit with 0, 1, 2^31 and 2^32 - 1 in each of the six words (iteration,
    group, parameter, purpose, chain, seed) in turn, and on 4096 counters of full-range words."""
    edges = (0, 1, 2 ** 31, 2 ** 32 - 1)
    base = (11, 5, 2, 1, 123456, 99)
    n = 0
    for word in range(6):
        for e in edges:
            k = list(base)
            k[word] = e
            ctr = numpy.array([k[:5]], dtype=numpy.uint32)
            out = _rng(gpu_lib, ctr, k[5], 2.0)
            ua, ub = ph.uniforms(*[numpy.array([v], dtype=numpy.uint64) for v in k])
            assert out[0, 1] == ua[0] and out[0, 2] == ub[0], (word, e, out[0], ua, ub)
            n += 1
    r = numpy.random.RandomState(77)
    ctr = r.randint(0, 2 ** 32, size=(4096, 5), dtype=numpy.uint64).astype(numpy.uint32)
    for seed in (2 ** 32 - 1, int(r.randint(0, 2 ** 32, dtype=numpy.uint64))):
        out = _rng(gpu_lib, ctr, seed, 2.0)
        ua, ub = ph.uniforms(ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3], ctr[:, 4], seed)
        assert numpy.array_equal(out[:, 1], ua) and numpy.array_equal(out[:, 2], ub)
    assert n == 24


@pytest.mark.parametrize("a", vr.GAMMA_SHAPES)
def test_gamma_draw_matches_oracle_and_distribution(gpu_lib, a):
    """Every one of the 20 000 draws within 1e-13 of the oracle's (the margin condition of
    tests/test_varmath_host.py rules out a legitimate difference of attempts), and the
    device's draws are Gamma(a): KS, mean and variance."""
    want, k, _ = vr.gamma_oracle(a)
    got = _rng(gpu_lib, vr.gamma_counters(), vr.GAMMA_SEED, a)[:, 3]
    rel = numpy.abs(got / want - 1.0)
    p, em, ev = vr.gamma_distribution_ok(got, a)
    print("VARMATH gamma device a = %-6g worst %.3e against the oracle (second attempts %d); "
          "KS p %.3f, mean off %.2f se, variance off %.2f se"
          % (a, rel.max(), int((k >= 1).sum()), p, em, ev))
    bad = numpy.flatnonzero(~(rel <= vr.GAMMA_RTOL))
    assert bad.size == 0, [(i, got[i], want[i], k[i]) for i in bad[:8]]
    assert p > vr.GAMMA_KS_P
    assert em <= 5.0 and ev <= 5.0


@pytest.mark.parametrize("G", vr.STREAM_G)
def test_hyper_rows_follow_the_stream(gpu_lib, G):
    fam, sizes = _gibbs_model(vr.STREAM_KIND, G)
    P, C, n = fam.n_params, vr.STREAM_C, vr.STREAM_ITERS
    kernel, modes = _gibbs_mode(fam, sizes)
    seed = 4000 + G
    ctr = vr.stream_counters(G, P)
    draws = _rng(gpu_lib, ctr.reshape(-1, 5), seed, (G - 1) / 2.0).reshape(n, P, C, 4)
    hz, g = draws[..., 0], draws[..., 3]
    for env in ({}, {"NMC_PERSIST": "0"}):
        what = (G, env)
        value, mu, s2 = go.start(C, P, G, seed)
        lp = rs.norm_logpdf(value, mu[:, :, None], numpy.sqrt(s2)[:, :, None])
        with _environ(env):
            eng = Engine(fam, sizes, C, "partial", None, seed=seed, chain_base=vr.STREAM_BASE)
        eng.set_state(value, lp, eng.eval_group_ll(value), mu, s2)
        eng.set_schedule(n, 0, 1, tune_interval=100)
        eng.run(0, n)
        eng.synchronize()
        rows = eng.samples()
        cfg = eng.launch_config()
        eng.close()
        if env:
            assert not cfg["persistent"] and cfg["kernel"].startswith("nmc_k_run<"), cfg
        else:
            assert cfg["kernel"].startswith(kernel) and cfg["mode"] in modes, (what, cfg)
        assert rows.shape[:2] == (C, n)
        vr.check_stream_rows(rows, s2, hz, g, G, P, what)
        print("VARMATH stream rows G=%-3d %-22s %d hyper draws tied to the stream"
              % (G, env or cfg["mode"], n * P * C))
