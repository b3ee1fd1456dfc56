#!/usr/bin/env python
"""Posterior predictive checks at the cfg-3 shape: 256 chains x 64 groups x 1000 observations,
partial pooling, LinearRegression.simple with known sigma, 200 recorded rows (3.3e9 draws).

(a) the device route: Engine.ppc() over the whole store -- host clock around the call (it ends
    in a synchronise and the copy of the partials) and the context's events around each kernel
    alone (nmc_ppc_partials: nmc_k_ppc_obs between slots 13 and 14, nmc_k_ppc_group with the
    merge of its slices between 14 and 15);
(b) the host route on the same store: the samples copied out (Engine.samples_raw, timed), then
    per recorded row numpy's generator (Generator.standard_normal) for the replicates of every
    (chain, observation) and the same statistics in numpy -- per observation the sums for the
    mean and M2 and the counts lt / eq, per group the mean, variance, minimum and maximum of
    every sample's replicate and the counts gt / eq -- over as many rows as fit --seconds; its
    time for all rows is a LINEAR EXTRAPOLATION from those rows, and the output says so
    ("b_extrapolated").
The two routes draw different numbers (Philox against numpy's PCG64), so parity is statistical:
the largest |p_a - p_b| over the groups and statistics, both over the rows (b) evaluated,
against the Monte Carlo standard error of the difference.  Prints one JSON line."""

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mcmc-for-nested-data_amd"))

import numpy  # noqa: E402

from nestmc import data, ppc  # noqa: E402
from nestmc.engine import Engine  # noqa: E402
from nestmc.families import LinearRegression  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=256)
    ap.add_argument("--groups", type=int, default=64)
    ap.add_argument("--obs", type=int, default=1000)
    ap.add_argument("--rows", type=int, default=200)
    ap.add_argument("--seconds", type=float, default=6.0, help="budget of route (b)")
    ap.add_argument("--repeat", type=int, default=3, help="timed calls of route (a)")
    a = ap.parse_args()
    C, G, N, R = a.chains, a.groups, a.obs, a.rows
    x, y, _, _ = data.linreg(G, N, seed=7)
    fam = LinearRegression.simple(x, y, sigma=1.0)
    eng = Engine(fam, [N] * G, C, "partial", None, seed=1)
    r = numpy.random.RandomState(0)
    value = numpy.array([0.0, 2.0])[None, :, None] + 0.1 * r.normal(size=(C, 2, G))
    eng.set_state(value, numpy.zeros((C, 2, G)), eng.eval_group_ll(value),
                  numpy.tile([0.0, 2.0], (C, 1)), numpy.full((C, 2), 0.5))
    eng.set_schedule(2 * R, R, 1)
    eng.run(0, 2 * R)
    eng.synchronize()
    assert eng.n_rows == R
    n_obs = G * N
    CB = (C + 63) // 64

    eng.ppc()                                    # warm up
    walls, k_obs, k_grp = [], [], []
    for _ in range(a.repeat):
        t0 = time.perf_counter()
        res = eng.ppc()
        walls.append(time.perf_counter() - t0)
        k_obs.append(eng.event_elapsed_ms(13, 14) * 1e-3)
        k_grp.append(eng.event_elapsed_ms(14, 15) * 1e-3)
    a_wall, a_obs, a_grp = (float(numpy.median(v)) for v in (walls, k_obs, k_grp))

    # (b) the host route on the same store
    t0 = time.perf_counter()
    raw = eng.samples_raw()                      # [rows][cols][C]
    b_copy = time.perf_counter() - t0
    pc = 2
    gen = numpy.random.default_rng(1)
    yv = numpy.asarray(y, dtype=numpy.float64)
    s1 = numpy.zeros(n_obs); s2 = numpy.zeros(n_obs)
    lt = numpy.zeros(n_obs, dtype=numpy.int64); eq = numpy.zeros(n_obs, dtype=numpy.int64)
    ty = ppc.stats_of(yv.reshape(G, N))          # [G, 4]
    gt = numpy.zeros((G, 4), dtype=numpy.int64); ge = numpy.zeros((G, 4), dtype=numpy.int64)
    t1 = numpy.zeros((G, 4)); t2 = numpy.zeros((G, 4))
    rows_b = 0
    t0 = time.perf_counter()
    while rows_b < R and (rows_b == 0 or time.perf_counter() - t0 < a.seconds):
        b0 = raw[rows_b, pc:pc + G].T                                   # [C][G]
        b1 = raw[rows_b, (G + pc) + pc:(G + pc) + pc + G].T
        yh = numpy.repeat(b0, N, axis=1) + numpy.repeat(b1, N, axis=1) * x[None, :]
        yrep = yh + gen.standard_normal(size=(C, n_obs))
        s1 += yrep.sum(axis=0); s2 += (yrep * yrep).sum(axis=0)
        lt += (yrep < yv).sum(axis=0); eq += (yrep == yv).sum(axis=0)
        g = yrep.reshape(C, G, N)
        T = numpy.stack([g.mean(axis=2), g.var(axis=2), g.min(axis=2), g.max(axis=2)], axis=2)
        gt += (T > ty).sum(axis=0); ge += (T == ty).sum(axis=0)
        t1 += T.sum(axis=0); t2 += (T * T).sum(axis=0)
        rows_b += 1
    b_rows_wall = time.perf_counter() - t0
    Sb = float(C * rows_b)
    p_b = (gt + ge / 2.0) / Sb
    b_all = b_copy + b_rows_wall * R / rows_b

    # statistical parity of the group p-values over the rows (b) evaluated: the same samples,
    # independent draws on either side
    p_a = eng.ppc(0, rows_b).p[:, 0, :]
    eng.close()
    se = numpy.sqrt(2.0 * numpy.maximum(p_a * (1 - p_a), 0.25 / Sb) / Sb)
    z = float(numpy.max(numpy.abs(p_a - p_b) / se))
    p_a = res.p[:, 0, :]
    draws = float(C) * R * n_obs
    print(json.dumps({
        "shape": {"chains": C, "groups": G, "obs_per_group": N, "rows": R, "draws": draws},
        "a_device_wall_s": a_wall, "a_kernel_obs_s": a_obs, "a_kernel_group_s": a_grp,
        "a_draws_per_s_obs_kernel": draws / a_obs, "a_draws_per_s_group_kernel": draws / a_grp,
        "a_group_slices": ppc.group_slices(R, G, 1, CB), "a_repeat": a.repeat,
        "b_copy_s": b_copy, "b_rows_evaluated": rows_b, "b_wall_s_those_rows": b_rows_wall,
        "b_extrapolated": rows_b < R, "b_wall_s_all_rows": b_all,
        "a_over_b_speedup": b_all / a_wall,
        "b_bytes_to_host": float(raw.nbytes),
        "a_bytes_to_host": float(CB) * (n_obs * (3 * 8 + 2 * 4) + G * 4 * (3 * 8 + 2 * 4)),
        "parity_max_abs_dp_over_se": z, "flagged_a": len(res.flagged()),
        "p_a_min": float(p_a.min()), "p_a_max": float(p_a.max())}))


if __name__ == "__main__":
    main()
