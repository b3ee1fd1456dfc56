#!/usr/bin/env python
"""WAIC at the cfg-3 shape: 256 chains x 64 groups x 1000 observations, partial pooling,
LinearRegression.simple with known sigma, 200 recorded rows (3.3e9 terms).

(a) the device route: Engine.waic() over the whole store -- host clock around the call (it
    ends in a synchronise and the copy of [CB, 5, n_obs]) and the context's events around the
    kernel alone (slots 14 / 15, nmc_waic_partials);
(b) the only route without nmc_k_waic, on the same store: Engine.obs_ll_rows in row batches
    and a numpy accumulation of the same 5-tuple on the host, over as many rows as fit
    --seconds; its time for all rows is a LINEAR EXTRAPOLATION from those rows.
Parity at the timed size: for 64 sampled observations, (a) and (b) over the rows (b)
evaluated, each against the longdouble formulas within Tol-lppd / Tol-M2 (tests/waic_ref.py).
Operation and byte counts come from the shapes; the instruction counts per row are those of
the compiled gfx950 loop body of nmc_k_waic<FamLinreg<2>> (see ISA below).  Prints one JSON
line."""

import argparse
import contextlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mcmc-for-nested-data_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy  # noqa: E402

import waic_ref  # noqa: E402
from nestmc import data, waic  # noqa: E402
from nestmc.engine import Engine  # noqa: E402
from nestmc.families import LinearRegression  # noqa: E402

# nmc_k_waic<FamLinreg<2>>, hipcc -O3 -ffp-contract=off --offload-arch=gfx950, the row loop's
# body (one sample row, T = 8 terms): 735 instructions, 623 VALU, 494 of them fp64
# (v_*_f64: obs_ll with its division, the range-reduced exp, the log-sum-exp and Welford
# updates), 8 scalar row loads of 16 B, 3 vector loads (the next row's theta and 1 / k)
ISA = {"T": 8, "instr_per_row": 735, "valu_per_row": 623, "fp64_per_row": 494}
# 256 CUs x 4 SIMDs x 16 fp64 lanes x 2.4 GHz (the 78.6 TFLOP/s fp64 vector
# peak counts an fma as two); HBM3E: 8.0 TB/s spec, 6.29 TB/s measured (MI355X_MICROARCH.md)
FP64_LANE_INSTR_PER_S = 256 * 4 * 16 * 2.4e9
HBM_BYTES_PER_S = 8.0e12


def batch_tuple(ll):
    """The 5-tuple of ll[S, n] (numpy, the from_ll_matrix formulas before their last step)."""
    m = ll.max(axis=0)
    mean = ll.mean(axis=0)
    d = ll - mean
    return numpy.stack([m, numpy.exp(ll - m).sum(axis=0), numpy.full(ll.shape[1], float(len(ll))),
                        mean, (d * d).sum(axis=0)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=256)
    ap.add_argument("--groups", type=int, default=64)
    ap.add_argument("--obs", type=int, default=1000)
    ap.add_argument("--rows", type=int, default=200)
    ap.add_argument("--seconds", type=float, default=4.0, help="budget of path (b)")
    ap.add_argument("--batch", type=int, default=2, help="rows per obs_ll_rows call of (b)")
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

    eng.waic()                                   # warm up
    t0 = time.perf_counter()
    res = eng.waic()
    a_wall = time.perf_counter() - t0
    a_kernel = eng.event_elapsed_ms(14, 15) * 1e-3

    # (b) row batches of the LL matrix to the host, accumulated there
    pick = numpy.random.RandomState(1).choice(n_obs, size=min(64, n_obs), replace=False)
    eng.obs_ll_rows(0, 1)                        # warm up
    acc, kept, rows_b = waic.identity(n_obs), [], 0
    t0 = time.perf_counter()
    while rows_b < R and (rows_b == 0 or time.perf_counter() - t0 < a.seconds):
        nb = min(a.batch, R - rows_b)
        ll = eng.obs_ll_rows(rows_b, nb).reshape(C * nb, n_obs)
        acc = waic.merge([acc, batch_tuple(ll)])
        kept.append(ll[:, pick].copy())
        rows_b += nb
    b_wall = time.perf_counter() - t0
    res_b = waic.finish(acc, eng.off)

    # parity over the rows (b) evaluated, on the sampled observations
    res_a = eng.waic(row_begin=0, n_rows=rows_b)
    llp = numpy.concatenate(kept, axis=0)
    off = [0, len(pick)]
    ratios = {}
    for name, rr in (("a", res_a), ("b", res_b)):
        sub = waic.WaicResult(rr.lppd_i[pick], rr.p_waic_i[pick], rr.n_samples, off)
        with contextlib.redirect_stdout(sys.stderr):
            ratios[name] = waic_ref.check(sub, llp, what="path (%s)" % name)
    eng.close()

    terms = float(C) * R * n_obs
    rows_waves = float(CB) * ((n_obs + ISA["T"] - 1) // ISA["T"]) * R   # (wave, row) pairs
    fp64 = rows_waves * ISA["fp64_per_row"] * 64                        # lane-instructions
    store_bytes = float(CB) * ((n_obs + ISA["T"] - 1) // ISA["T"]) * R * 2 * 64 * 8
    obs_bytes = rows_waves * ISA["T"] * 2 * 8
    out_bytes = float(CB) * 5 * n_obs * 8
    t_fp64 = fp64 / FP64_LANE_INSTR_PER_S
    t_hbm = (R * 2 * (G + 2) * C * 8 + n_obs * 16 + out_bytes) / HBM_BYTES_PER_S
    b_all = b_wall * R / rows_b
    print(json.dumps({
        "shape": {"chains": C, "groups": G, "obs_per_group": N, "rows": R, "terms": terms},
        "a_device_wall_s": a_wall, "a_kernel_s": a_kernel,
        "a_terms_per_s_wall": terms / a_wall, "a_terms_per_s_kernel": terms / a_kernel,
        "b_rows_evaluated": rows_b, "b_wall_s_those_rows": b_wall,
        "b_wall_s_all_rows_extrapolated": b_all, "b_terms_per_s": terms / b_all,
        "a_over_b_speedup_extrapolated": b_all / a_wall,
        "b_bytes_to_host_all_rows": terms * 8, "a_bytes_to_host": out_bytes,
        "kernel_fp64_lane_instr": fp64,
        "kernel_fp64_instr_per_term": ISA["fp64_per_row"] / ISA["T"],
        "kernel_instr_per_term": ISA["instr_per_row"] / ISA["T"],
        "kernel_store_bytes_requested": store_bytes, "kernel_obs_bytes_requested": obs_bytes,
        "kernel_min_s_fp64_peak": t_fp64, "kernel_min_s_hbm_compulsory": t_hbm,
        "kernel_bound": "fp64 vector issue" if t_fp64 > t_hbm else "HBM",
        "kernel_share_of_fp64_peak": t_fp64 / a_kernel,
        "parity_rows": rows_b, "parity_obs": len(pick),
        "parity_a_err_over_tol_lppd_M2": ratios["a"], "parity_b_err_over_tol_lppd_M2": ratios["b"],
        "waic": res.waic, "se_waic": res.se_waic, "p_waic": res.p_waic}))


if __name__ == "__main__":
    main()
