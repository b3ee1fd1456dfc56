#!/usr/bin/env python
"""Held-out and new-group prediction at the cfg-3 shape: 256 chains x 64 groups x 1000
observations, partial pooling, LinearRegression.simple with known sigma, 200 recorded rows; the
new table has 100 rows for each of the 64 training groups plus 10 new groups of 100 rows
(7 400 new rows, every fourth without a response).

(a) the device route: Engine.predict() over the whole store -- host clock around the call (it
    ends in a synchronise and the copy of the partials) and the context's events 16 / 17 around
    nmc_k_predict alone;
(b) the host route on the same inputs: the samples copied out (Engine.samples_raw, timed), then
    per recorded row the new groups' values and the draws from numpy's generator
    (Generator.standard_normal), the log densities, and at the end nestmc.predict.from_draws
    over the rows evaluated -- as many rows as fit --seconds and --max-rows; its time for all
    rows is a LINEAR EXTRAPOLATION from those rows, and the output says so ("b_extrapolated").
The two routes draw different numbers (Philox against numpy's PCG64), so parity is statistical:
elpd_test of both over the rows (b) evaluated, in units of its standard error, and over the
training groups alone (no random theta there) the largest |lpd_a - lpd_b|.  Prints one JSON
line."""

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mcmc-for-nested-data_amd"))

import numpy  # noqa: E402

from nestmc import NewData, data, predict  # noqa: E402
from nestmc.engine import Engine  # noqa: E402
from nestmc.families import LinearRegression  # noqa: E402

LOG_C = 0.5 * numpy.log(2.0 * numpy.pi)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=256)
    ap.add_argument("--groups", type=int, default=64)
    ap.add_argument("--obs", type=int, default=1000)
    ap.add_argument("--rows", type=int, default=200)
    ap.add_argument("--new-per-group", type=int, default=100)
    ap.add_argument("--new-groups", type=int, default=10)
    ap.add_argument("--seconds", type=float, default=6.0, help="budget of route (b)")
    ap.add_argument("--max-rows", type=int, default=16,
                    help="most rows of route (b): it keeps their draws (S x n_new doubles)")
    ap.add_argument("--repeat", type=int, default=3, help="timed calls of route (a)")
    a = ap.parse_args()
    C, G, N, R, M, K = a.chains, a.groups, a.obs, a.rows, a.new_per_group, a.new_groups
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
    codes = numpy.concatenate([numpy.repeat(numpy.arange(G), M),
                               numpy.repeat(-1 - numpy.arange(K), M)]).astype(numpy.int32)
    n_new = len(codes)
    xn = r.normal(size=n_new)
    yn = 2.0 * xn + r.normal(size=n_new)
    yn[::4] = numpy.nan
    new = NewData(numpy.stack([xn, yn], 1), codes)
    eng.set_new_data(new)
    CB = (C + 63) // 64

    eng.predict()                                # warm up
    walls, kern = [], []
    for _ in range(a.repeat):
        t0 = time.perf_counter()
        res = eng.predict()
        walls.append(time.perf_counter() - t0)
        kern.append(eng.event_elapsed_ms(16, 17) * 1e-3)
    a_wall, a_kern = float(numpy.median(walls)), float(numpy.median(kern))

    # (b) the host route on the same store
    t0 = time.perf_counter()
    raw = eng.samples_raw()                      # [rows][cols][C]
    b_copy = time.perf_counter() - t0
    gen = numpy.random.default_rng(1)
    train = codes >= 0
    gi = numpy.where(train, codes, 0)
    ki = numpy.where(train, 0, -(codes + 1))
    yreps, lls = [], []
    rows_b = 0
    t0 = time.perf_counter()
    while rows_b < min(R, a.max_rows) and (rows_b == 0 or time.perf_counter() - t0 < a.seconds):
        row = raw[rows_b]                                               # [cols][C]
        th = []
        for q in range(2):
            base = q * (G + 2)
            tnew = row[base][:, None] + numpy.sqrt(row[base + 1])[:, None] \
                * gen.standard_normal(size=(C, K))
            th.append(numpy.where(train[None, :], row[base + 2:base + 2 + G].T[:, gi],
                                  tnew[:, ki]))
        yh = th[0] + th[1] * xn[None, :]
        yreps.append(yh + gen.standard_normal(size=(C, n_new)))
        t = yh - yn[None, :]
        lls.append(-(t * t) / 2.0 - LOG_C)
        rows_b += 1
    Sb = C * rows_b
    yrep = numpy.stack(yreps, 1).reshape(Sb, n_new, 1)
    ll = numpy.stack(lls, 1).reshape(Sb, n_new)
    host = predict.from_draws(yrep, ll, yn, codes)
    b_rows_wall = time.perf_counter() - t0
    b_all = b_copy + b_rows_wall * R / rows_b

    dev = eng.predict(0, rows_b)
    eng.close()
    has = dev.has_response
    tr = has & train
    print(json.dumps({
        "shape": {"chains": C, "groups": G, "obs_per_group": N, "rows": R, "n_new": n_new,
                  "new_groups": K, "with_response": int(has.sum())},
        "a_device_wall_s": a_wall, "a_kernel_s": a_kern, "a_repeat": a.repeat,
        "a_terms_per_s": float(C) * R * n_new / a_kern,
        "b_copy_s": b_copy, "b_rows_evaluated": rows_b, "b_wall_s_those_rows": b_rows_wall,
        "b_extrapolated": rows_b < R, "b_wall_s_all_rows": b_all,
        "a_over_b_speedup": b_all / a_wall,
        "b_bytes_to_host": float(raw.nbytes),
        "a_bytes_to_host": float(CB) * n_new * (2 * 8 + 3 * 8 + 2 * 4),
        "elpd_test": res.elpd_test, "se": res.se,
        "parity_elpd_a": dev.elpd_test, "parity_elpd_b": host.elpd_test,
        "parity_elpd_diff_over_se": abs(dev.elpd_test - host.elpd_test) / dev.se,
        "parity_training_max_abs_dlpd": float(numpy.max(numpy.abs(dev.lpd_i[tr] - host.lpd_i[tr]))),
        "parity_max_abs_dmean_over_sd": float(numpy.max(
            numpy.abs(dev.mean_i - host.mean_i) / (dev.sd_i / numpy.sqrt(Sb))))}))


if __name__ == "__main__":
    main()
