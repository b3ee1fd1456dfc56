#!/usr/bin/env python
"""PSIS-LOO at the cfg-3 shape: 256 chains x 64 groups x 1000 observations, partial pooling,
LinearRegression.simple with known sigma, 200 recorded rows: 64 000 observations of
S = 51 200 samples each (3.3e9 log-likelihood terms, M = 679 tail candidates).

(a) the device route: Engine.loo() over the whole store -- host clock around the call (the
    buffers' allocation, every batch's nmc_k_loo_ll, sort and nmc_k_psis, the copy of the
    per-observation results) and the context's events around the kernels alone (slots 8 / 9,
    nmc_loo).  The split per kernel comes from a kernel trace of this program with nothing
    else traced,
      rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- \\
          python tools/loobench.py --only-a
    and then --kernel-stats DIR on a second run, which reads the trace's per-kernel totals;
(b) the route without these kernels, on the same store: Engine.obs_ll_rows in row batches (the
    whole [S, n_obs] matrix crosses to the host, 26 GB) and nestmc.loo.from_ll_matrix.  Its
    time is a LINEAR EXTRAPOLATION: obs_ll_rows is timed over --ll-rows rows and scaled to all
    rows; from_ll_matrix is timed on 64 sampled observations and scaled to all of them.
Parity on the 64 sampled observations: (a) against the longdouble reference within the
tolerances of tests/psis_ref.py, and (a) against (b).  Prints one JSON line."""

import argparse
import contextlib
import csv
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mcmc-for-nested-data_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy  # noqa: E402

import psis_ref  # noqa: E402
from nestmc import data, loo  # noqa: E402
from nestmc.engine import Engine  # noqa: E402
from nestmc.families import LinearRegression  # noqa: E402

KERNELS = ("nmc_k_loo_ll", "nmc_k_sort_tiles", "nmc_k_sort_merge", "nmc_k_psis")


def read_stats(directory):
    """{kernel: (calls, total seconds)} of a rocprofv3 --kernel-trace --stats run."""
    out = {}
    for fn in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
        with open(fn) as f:
            for row in csv.DictReader(f):
                for k in KERNELS:
                    if k in row["Name"]:
                        c, t = out.get(k, (0, 0.0))
                        out[k] = (c + int(row["Calls"]), t + int(row["TotalDurationNs"]) * 1e-9)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=256)
    ap.add_argument("--groups", type=int, default=64)
    ap.add_argument("--obs", type=int, default=1000)
    ap.add_argument("--rows", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ll-rows", type=int, default=8, help="rows of obs_ll_rows timed for (b)")
    ap.add_argument("--only-a", action="store_true", help="one Engine.loo() and nothing else")
    ap.add_argument("--kernel-stats", default=None,
                    help="directory of a rocprofv3 --kernel-trace --stats run of --only-a")
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
    n_obs, S = G * N, C * R

    if a.only_a:
        res = eng.loo()
        eng.close()
        print(json.dumps({"only_a": True, "elpd": res.elpd, "n_bad": res.n_bad}))
        return

    eng.loo()                                    # warm up
    a_wall, a_kernel = [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        res = eng.loo()
        a_wall.append(time.perf_counter() - t0)
        a_kernel.append(eng.event_elapsed_ms(8, 9) * 1e-3)

    # (b) the matrix to the host in row batches; from_ll_matrix on 64 sampled observations
    pick = numpy.sort(numpy.random.RandomState(1).choice(n_obs, size=min(64, n_obs),
                                                         replace=False))
    eng.obs_ll_rows(0, 1)                        # warm up
    nb = 2
    t0 = time.perf_counter()
    for q in range(0, min(a.ll_rows, R), nb):
        eng.obs_ll_rows(q, min(nb, R - q))
    b_ll = time.perf_counter() - t0
    b_ll_rows = min(a.ll_rows, R)
    # the sampled observations' columns over all rows (not timed: only their values are needed)
    kept = [eng.obs_ll_rows(q, min(nb, R - q))[:, :, pick] for q in range(0, R, nb)]
    llp = numpy.concatenate(kept, axis=1)                       # [C, R, 64]
    mat = numpy.ascontiguousarray(numpy.transpose(llp, (1, 0, 2))).reshape(S, len(pick))
    t0 = time.perf_counter()
    res_b = loo.from_ll_matrix(mat, [0, len(pick)])
    b_fit = time.perf_counter() - t0
    eng.close()

    worst = {"elpd": 0.0, "lppd": 0.0, "k": 0.0}
    with contextlib.redirect_stdout(sys.stderr):
        for j, i in enumerate(pick):
            ref = psis_ref.check("obs%d" % i, mat[:, j], res.elpd_i[i], res.lppd_i[i],
                                 res.pareto_k[i], res.n_tail[i], what="path (a)")
            tk, _, te, tl = psis_ref.tolerances(ref, S)
            L = numpy.longdouble
            worst["elpd"] = max(worst["elpd"], float(abs(L(res.elpd_i[i]) - ref["elpd"]) / te))
            worst["lppd"] = max(worst["lppd"], float(abs(L(res.lppd_i[i]) - ref["lppd"]) / tl))
            if tk > 0:
                worst["k"] = max(worst["k"], float(abs(L(res.pareto_k[i]) - ref["k"]) / tk))
    ab = {"elpd": float(numpy.max(numpy.abs(res.elpd_i[pick] - res_b.elpd_i))),
          "k": float(numpy.max(numpy.abs(res.pareto_k[pick] - res_b.pareto_k))),
          "n_tail_equal": bool(numpy.array_equal(res.n_tail[pick], res_b.n_tail))}

    m = lambda v: float(numpy.median(v))   # noqa: E731
    b_ll_all = b_ll * R / b_ll_rows
    b_fit_all = b_fit * n_obs / len(pick)
    out = {
        "shape": {"chains": C, "groups": G, "obs_per_group": N, "rows": R, "n_obs": n_obs,
                  "samples_per_obs": S, "tail_candidates": loo.tail_length(S),
                  "terms": float(S) * n_obs},
        "a_wall_s": a_wall, "a_kernels_s_events": a_kernel,
        "b_obs_ll_rows_s": b_ll, "b_obs_ll_rows_timed": b_ll_rows,
        "b_obs_ll_rows_s_all_rows_extrapolated": b_ll_all,
        "b_from_ll_matrix_s_64_obs": b_fit,
        "b_from_ll_matrix_s_all_obs_extrapolated": b_fit_all,
        "b_wall_s_extrapolated": b_ll_all + b_fit_all,
        "a_over_b_speedup_extrapolated": (b_ll_all + b_fit_all) / m(a_wall),
        "b_bytes_to_host": float(S) * n_obs * 8, "a_bytes_to_host": n_obs * 36.0,
        "parity_obs": len(pick), "parity_a_err_over_tol": worst, "parity_a_minus_b_max_abs": ab,
        "elpd": res.elpd, "se": res.se, "p_loo": res.p_loo, "n_bad": res.n_bad,
        "k_max": float(numpy.max(res.pareto_k)),
    }
    if a.kernel_stats:
        st = read_stats(a.kernel_stats)
        out["a_kernel_split_rocprofv3"] = {k: {"calls": c, "total_s": t} for k, (c, t) in st.items()}
    with contextlib.suppress(BrokenPipeError):
        print(json.dumps(out))


if __name__ == "__main__":
    main()
