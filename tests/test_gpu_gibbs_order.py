"""GPU: the Gibbs update sums in numpy's order, bit for bit.

csrc/special.h and DESIGN claim that the hyper mean and the sum of squares are summed as
numpy.sum sums them (8 accumulators per leaf of at most 128, leaves merged pairwise), so that
the hyper-parameters equal the reference's bit for bit.  The order has several
implementations (nmc_hyper_streams + nmc_hyper_combine, nmc_hyper_compute, nmc_pairwise_reg,
nmc_pairwise_stream, the closing updates), chosen by G, by the parity of C (nmc_hyper_dma /
nmc_hyper_load) and by NMC_PERSIST; the oracle tests hold them to 1e-9, which a sequential
sum or a wrong merge order passes.

Replay mode makes the order checkable exactly: the hyper variates are the test's own inputs
and the library is built without contraction.  From the device's OWN recorded row i, which
holds each parameter's mu, s2 and the values x its Gibbs update read:

* mu == numpy.sum(x) / G + numpy.sqrt(s2_prev / G) * hz, bit for bit, every chain;
* s2 == r * scale with scale = a * (numpy.sum((x - mu)**2) / (G - 1)), a = (G - 1) / 2, bit
  for bit for ONE double r shared by all chains (the device's 1 / gammainccinv(a, u): every
  chain replays the same u), and r within 1e-12 of scipy's (the igamci tolerance of
  tests/test_gpu_parity.py, plus 2 ulp for the reciprocal).

The start values span magnitudes (normal * exp(2 normal)), so that the order shows in the
bits: the test asserts that at least 20 % of the sums it checks differ from their
sequential sum (G >= 8; below, numpy's order is the sequential one).
"""

import numpy
import pytest

import gibbs_order as go
from nestmc.engine import Engine
from oracle import restatement as rs
from rowpath_cases import environ as _environ, gibbs_mode as _gibbs_mode, \
    gibbs_model as _gibbs_model

pytestmark = pytest.mark.gpu

N_ITER = 4
G_LIST = [2, 3, 7, 8, 9, 63, 64, 65, 120, 121, 127, 128, 129, 136, 512, 513]


def _replay_rows(fam, sizes, C, env, seed):
    """Four replayed iterations from a start of spread magnitudes: (rows [C, 4, cols], start
    s2 [C, P], hz [C, 4, P], hu [4, P], launch config)."""
    G, P = len(sizes), fam.n_params
    value, mu, s2 = go.start(C, P, G, seed)
    lp = rs.norm_logpdf(value, mu[:, :, None], numpy.sqrt(s2)[:, :, None])
    z, u, hz, hu = go.variates(C, P, G, N_ITER, seed)
    with _environ(env):
        eng = Engine(fam, sizes, C, "partial", None, rng="replay")
    eng.set_state(value, lp, eng.eval_group_ll(value), mu, s2)
    eng.set_replay(z, u, hz, numpy.broadcast_to(hu[None], (C, N_ITER, P)).copy())
    eng.set_schedule(N_ITER, 0, 1, tune_interval=100)
    eng.run(0, N_ITER)
    eng.synchronize()
    rows = eng.samples()
    cfg = eng.launch_config()
    eng.close()
    return rows, s2, hz, hu, cfg


@pytest.mark.parametrize("G", G_LIST)
@pytest.mark.parametrize("kind", ["linreg2", "gauss1"])
def test_gibbs_sums_in_numpy_order(gpu_lib, kind, G):
    fam, sizes = _gibbs_model(kind, G)
    P = fam.n_params
    kernel, modes = _gibbs_mode(fam, sizes)
    for C in (65, 66) if G in (8, 9, 64, 128) else (65,):
        for env in ({}, {"NMC_PERSIST": "0"}):
            what = (kind, G, C, env)
            rows, s2_start, hz, hu, cfg = _replay_rows(fam, sizes, C, env, 100 * G + C)
            if env:
                assert not cfg["persistent"] and cfg["kernel"].startswith("nmc_k_run<"), cfg
            else:
                assert cfg["kernel"].startswith(kernel) and cfg["mode"] in modes, (what, cfg)
            share = go.check(rows, s2_start, hz, hu, G, P, what)
            print("GIBBS ORDER %-8s G=%-3d C=%d %-22s sums that differ from sequential: %.2f"
                  % (kind, G, C, env or cfg["mode"], share))
            if G >= 8:
                assert share >= 0.20, (what, share)
            else:
                assert share == 0.0, (what, share)
