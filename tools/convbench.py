#!/usr/bin/env python
"""Convergence diagnostics at the cfg-3 store shape: 256 chains x 132 columns (64 groups, two
parameters, partial pooling) x 200 recorded rows, n = 100 rows per half-chain.

(a) the device route: Engine.convergence() over the whole store -- host clock around the call
    (kernel, the copy of vg / mean / m2, merge and finish on the host) and the context's events
    around nmc_k_conv alone (slots 12 / 13, nmc_conv_partials);
(b) the only route without nmc_k_conv, on the same store: Engine.samples() -> x[K][m][n] ->
    nestmc.convergence.from_halfchains; its nmc_variogram call (timed on its own as well)
    includes the copy of x to the device;
(c) nmc_k_variogram alone: from a kernel trace of this program,
      rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/convbench.py
    and then --kernel-trace DIR on a second run, which reads every dispatch's duration.
(a) and (b) alternate --reps times in one process.  Parity: (a) against (b) within the bounds
of tests/convergence_ref.py on every column.  Counts come from the shapes; the instruction
counts per term are those of the compiled gfx950 loop of nmc_k_conv (ISA below).  Prints one
JSON line."""

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

import convergence_ref as cr  # noqa: E402
from nestmc import convergence as conv  # noqa: E402
from nestmc import data, diagnosis  # noqa: E402
from nestmc.engine import Engine  # noqa: E402
from nestmc.families import LinearRegression  # noqa: E402

# nmc_k_conv, hipcc -O3 -ffp-contract=off --offload-arch=gfx950: the main loop (two blocks of
# 8 rows x 8 lags = 128 terms) is 622 instructions: 384 v_*_f64 (sub, mul, add per term), 40
# other VALU (the two row pointers' steps), 32 global loads (2 per 8 terms, 512 B each per
# wave), 163 scalar (the steps' clamps, the waits)
ISA = {"L": 8, "terms_per_loop": 128, "instr_per_loop": 622, "fp64_per_loop": 384,
       "valu_per_loop": 424, "loads_per_loop": 32, "salu_per_loop": 163}
# 256 CUs x 4 SIMDs x 16 fp64 lanes x 2.4 GHz
FP64_LANE_INSTR_PER_S = 256 * 4 * 16 * 2.4e9


def read_trace(directory):
    """{kernel name prefix: [durations in s]} of a rocprofv3 kernel trace under directory."""
    out = {"nmc_k_conv": [], "nmc_k_variogram": []}
    for fn in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        with open(fn) as f:
            for row in csv.DictReader(f):
                for k in out:
                    if k in row["Kernel_Name"]:
                        out[k].append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"]))
                                      * 1e-9)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=256)
    ap.add_argument("--groups", type=int, default=64)
    ap.add_argument("--obs", type=int, default=100)
    ap.add_argument("--rows", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kernel-trace", default=None,
                    help="directory of a rocprofv3 --kernel-trace run of this program")
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
    cols, n, CB = eng.cols, R // 2, (C + 63) // 64

    def route_b():
        t0 = time.perf_counter()
        xh = conv.halfchains(eng.samples())
        t1 = time.perf_counter()
        diagnosis.variogram(xh)                  # (timed alone; from_halfchains calls it again)
        t2 = time.perf_counter()
        res = conv.from_halfchains(xh)
        return res, xh, (time.perf_counter() - t2) + (t1 - t0), t2 - t1

    eng.convergence()                            # warm up
    route_b()
    a_wall, a_kernel, b_wall, b_vario = [], [], [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        res_a = eng.convergence()
        a_wall.append(time.perf_counter() - t0)
        a_kernel.append(eng.event_elapsed_ms(12, 13) * 1e-3)
        res_b, xh, w, v = route_b()
        b_wall.append(w)
        b_vario.append(v)
    eng.close()

    tol = cr.tolerances(xh, CB)
    ratios = {}
    for k in ("V", "rhat", "mean", "sd"):
        err = numpy.abs(getattr(res_a, k) - getattr(res_b, k))
        t = numpy.asarray(tol[k], dtype=numpy.float64)
        ratios[k] = float(numpy.max(err[t > 0] / t[t > 0]))
    same_T = bool(numpy.array_equal(res_a.T, res_b.T))
    rel = numpy.abs(res_a.effective_n - res_b.effective_n) / numpy.abs(res_b.effective_n)
    ratios["effective_n"] = float(numpy.max(rel / tol["neff_rel"](res_b.T, res_b.effective_n)))

    terms = float(C) * cols * n * (n - 1)
    med = lambda v: float(numpy.median(v))   # noqa: E731
    out = {
        "shape": {"chains": C, "columns": cols, "rows": R, "n": n, "pair_terms": terms},
        "a_wall_s": a_wall, "a_kernel_s_events": a_kernel,
        "b_wall_s": b_wall, "b_nmc_variogram_s_incl_copy": b_vario,
        "b_bytes_to_host_and_back": 2 * 8.0 * C * cols * R,
        "a_bytes_to_host": 8.0 * (CB * cols * n + 4 * cols * C),
        "wall_a_over_b": med(a_wall) / med(b_wall),
        "kernel_fp64_instr_per_term": ISA["fp64_per_loop"] / ISA["terms_per_loop"],
        "kernel_valu_instr_per_term": ISA["valu_per_loop"] / ISA["terms_per_loop"],
        "kernel_loads_per_term": ISA["loads_per_loop"] / ISA["terms_per_loop"],
        "kernel_bytes_requested": terms / 64 * ISA["loads_per_loop"] / ISA["terms_per_loop"] * 512,
        "kernel_requested_bytes_per_s": terms / 64 * ISA["loads_per_loop"]
        / ISA["terms_per_loop"] * 512 / med(a_kernel),
        "kernel_min_s_fp64_peak": 3 * terms / FP64_LANE_INSTR_PER_S,
        "kernel_share_of_fp64_peak": 3 * terms / FP64_LANE_INSTR_PER_S / med(a_kernel),
        "parity_err_over_bound": ratios, "parity_same_cutoff": same_T,
        "columns_converged": int(numpy.sum(res_a.converged)),
        "columns_enough_n": int(numpy.sum(res_a.enough_n)),
    }
    if a.kernel_trace:
        tr = read_trace(a.kernel_trace)
        # (the trace holds the warm-up dispatches too: the last --reps of each kernel; route
        # (b) launches nmc_k_variogram twice per repetition)
        c = tr["nmc_k_variogram"][-2 * a.reps:]
        ak = tr["nmc_k_conv"][-a.reps:]
        out.update({"c_nmc_k_variogram_s_trace": c, "a_nmc_k_conv_s_trace": ak,
                    "c_spread_s": (max(c) - min(c)) if c else None,
                    "kernel_a_over_c_trace": med(ak) / med(c) if c and ak else None,
                    "kernel_a_events_over_c_trace": med(a_kernel) / med(c) if c else None})
    with contextlib.suppress(BrokenPipeError):
        print(json.dumps(out))


if __name__ == "__main__":
    main()
