#!/usr/bin/env python
"""LOO-PIT and the leave-one-out predictive moments at the cfg-3 shape: 256 chains x 64 groups
x 1000 observations, partial pooling, LinearRegression.simple with known sigma, 200 recorded
rows: 64 000 observations of S = 51 200 samples each (3.3e9 log-likelihood terms and as many
replicates, M = 679 tail candidates).

(a) the device route: Engine.loo_pit() over the whole store -- host clock around the call (the
    buffers' allocation, every batch's nmc_k_loo_ll, sort, nmc_k_psis, nmc_k_loo_yrep and
    nmc_k_psis_expect, the copy of the per-observation results) and the context's events
    around the kernels alone (slots 8 / 9, nmc_loo_pit);
(l) Engine.loo() of the same build on the same store, the same way: (a) - (l) is what the
    extra draw and expectation passes cost.  The split per kernel comes from a kernel trace
    of this program with nothing else traced,
      rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- \\
          python tools/loopitbench.py --only-a
    and then --kernel-stats DIR on a second run, which reads the trace's per-kernel totals;
(b) the route without these kernels, on the same store: Engine.obs_ll_rows and
    Engine.predictive_draws in row batches (both [S, n_obs] matrices cross to the host, 26 GB
    each) and nestmc.loopit.from_matrices.  Its time is a LINEAR EXTRAPOLATION: the two
    downloads are timed over --ll-rows rows and scaled to all rows; from_matrices is timed on
    64 sampled observations and scaled to all of them.
Parity on the 64 sampled observations: (a) against the longdouble reference within the
tolerances of tests/loopit_ref.py, and (a) against (b).  Prints one JSON line."""

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

import loopit_ref  # noqa: E402
from nestmc import data, loo, loopit  # noqa: E402
from nestmc.engine import Engine  # noqa: E402
from nestmc.families import LinearRegression  # noqa: E402

KERNELS = ("nmc_k_loo_ll", "nmc_k_loo_yrep", "nmc_k_sort_tiles", "nmc_k_sort_merge",
           "nmc_k_psis_expect", "nmc_k_psis")


def read_stats(directory):
    """{kernel: (calls, total seconds)} of a rocprofv3 --kernel-trace --stats run."""
    out = {}
    for fn in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
        with open(fn) as f:
            for row in csv.DictReader(f):
                for k in KERNELS:        # (nmc_k_psis_expect before its prefix nmc_k_psis)
                    if k in row["Name"]:
                        c, t = out.get(k, (0, 0.0))
                        out[k] = (c + int(row["Calls"]), t + int(row["TotalDurationNs"]) * 1e-9)
                        break
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=256)
    ap.add_argument("--groups", type=int, default=64)
    ap.add_argument("--obs", type=int, default=1000)
    ap.add_argument("--rows", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ll-rows", type=int, default=8, help="rows of the downloads timed for (b)")
    ap.add_argument("--only-a", action="store_true", help="one Engine.loo_pit() and nothing else")
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
        res = eng.loo_pit()
        eng.close()
        print(json.dumps({"only_a": True, "n_outside": res.n_outside, "ks": res.ks}))
        return

    eng.loo_pit()                                # warm up
    eng.loo()
    a_wall, a_kernel, l_wall, l_kernel = [], [], [], []
    for _ in range(a.reps):                      # alternated
        t0 = time.perf_counter()
        res = eng.loo_pit()
        a_wall.append(time.perf_counter() - t0)
        a_kernel.append(eng.event_elapsed_ms(8, 9) * 1e-3)
        t0 = time.perf_counter()
        res_l = eng.loo()
        l_wall.append(time.perf_counter() - t0)
        l_kernel.append(eng.event_elapsed_ms(8, 9) * 1e-3)
    same_loo = bool(res.loo.elpd_i.tobytes() == res_l.elpd_i.tobytes()
                    and res.loo.pareto_k.tobytes() == res_l.pareto_k.tobytes())

    # (b) both matrices to the host in row batches; from_matrices on 64 sampled observations
    pick = numpy.sort(numpy.random.RandomState(1).choice(n_obs, size=min(64, n_obs),
                                                         replace=False))
    eng.obs_ll_rows(0, 1)                        # warm up
    eng.predictive_draws(0, 1)
    nb = 2
    t0 = time.perf_counter()
    for q in range(0, min(a.ll_rows, R), nb):
        eng.obs_ll_rows(q, min(nb, R - q))
        eng.predictive_draws(q, min(nb, R - q))
    b_dl = time.perf_counter() - t0
    b_dl_rows = min(a.ll_rows, R)
    # the sampled observations' columns over all rows (not timed: only their values are needed)
    kl = [eng.obs_ll_rows(q, min(nb, R - q))[:, :, pick] for q in range(0, R, nb)]
    ky = [eng.predictive_draws(q, min(nb, R - q))[:, :, pick, 0] for q in range(0, R, nb)]
    yobs = eng.observed()[pick, 0]
    eng.close()
    flat = lambda k: numpy.ascontiguousarray(   # noqa: E731
        numpy.transpose(numpy.concatenate(k, axis=1), (1, 0, 2))).reshape(S, len(pick))
    mat, rep = flat(kl), flat(ky)
    t0 = time.perf_counter()
    res_b = loopit.from_matrices(mat, rep, yobs, [0, len(pick)])
    b_fit = time.perf_counter() - t0

    worst = {}
    with contextlib.redirect_stdout(sys.stderr):
        for j, i in enumerate(pick):
            got = dict(ess=res.ess[i], wlt=res.wlt[i, 0], weq=res.weq[i, 0],
                       mean=res.loo_mean[i, 0], var=res.loo_var[i, 0], n_tail=res.loo.n_tail[i])
            err = loopit_ref.check_values("obs%d" % i, mat[:, j], rep[:, j], yobs[j], got,
                                          what="path (a)")
            for k, v in err.items():
                worst[k] = max(worst.get(k, 0.0), v)
    ab = {"loo_pit": float(numpy.max(numpy.abs(res.loo_pit[pick] - res_b.loo_pit))),
          "loo_mean": float(numpy.max(numpy.abs(res.loo_mean[pick] - res_b.loo_mean))),
          "loo_sd": float(numpy.max(numpy.abs(res.loo_sd[pick] - res_b.loo_sd))),
          "ess_rel": float(numpy.max(numpy.abs(res.ess[pick] / res_b.ess - 1.0)))}

    m = lambda v: float(numpy.median(v))   # noqa: E731
    b_dl_all = b_dl * R / b_dl_rows
    b_fit_all = b_fit * n_obs / len(pick)
    out = {
        "shape": {"chains": C, "groups": G, "obs_per_group": N, "rows": R, "n_obs": n_obs,
                  "samples_per_obs": S, "tail_candidates": loo.tail_length(S),
                  "terms": float(S) * n_obs},
        "a_wall_s": a_wall, "a_kernels_s_events": a_kernel,
        "loo_wall_s": l_wall, "loo_kernels_s_events": l_kernel,
        "a_over_loo_wall": m(a_wall) / m(l_wall),
        "a_minus_loo_kernels_s": m(a_kernel) - m(l_kernel),
        "loo_fields_bit_identical_to_engine_loo": same_loo,
        "b_downloads_s": b_dl, "b_download_rows_timed": b_dl_rows,
        "b_downloads_s_all_rows_extrapolated": b_dl_all,
        "b_from_matrices_s_64_obs": b_fit,
        "b_from_matrices_s_all_obs_extrapolated": b_fit_all,
        "b_wall_s_extrapolated": b_dl_all + b_fit_all,
        "a_over_b_speedup_extrapolated": (b_dl_all + b_fit_all) / m(a_wall),
        "b_bytes_to_host": 2.0 * S * n_obs * 8, "a_bytes_to_host": n_obs * 84.0,
        "parity_obs": len(pick), "parity_a_err_over_tol": worst, "parity_a_minus_b_max_abs": ab,
        "n_outside": res.n_outside, "frac_outside": res.frac_outside, "ks": res.ks,
        "ess_min": float(numpy.min(res.ess)), "ess_median": float(numpy.median(res.ess)),
        "k_max": float(numpy.max(res.pareto_k)),
    }
    if a.kernel_stats:
        st = read_stats(a.kernel_stats)
        out["a_kernel_split_rocprofv3"] = {k: {"calls": c, "total_s": t} for k, (c, t) in st.items()}
    with contextlib.suppress(BrokenPipeError):
        print(json.dumps(out))


if __name__ == "__main__":
    main()
