#!/usr/bin/env python
"""Posterior comoments (covariance / correlation matrix of all columns) at the cfg-3 and cfg-4
store shapes: two parameters under partial pooling, 64 groups x 256 chains x 200 recorded rows
(S = 51 200 samples, 132 columns) and 256 groups x 1 024 chains x 200 rows (S = 204 800, 516
columns, 845 MB).  The store is written with nmc_debug_set_samples (column offsets and scales
plus noise; no sampling).

(a) the device route: Engine.comoments() over the whole store -- host clock around the call
    (allocation of M and the partial tiles, the three kernels, the copy of M and the moments)
    and the context's events around the kernels alone (slots 2 / 3, nmc_comoments);
(b) the host route on the same store: Engine.samples_raw() (the copy of the whole store) plus
    the leanest numpy formulation -- one transposing copy to [cols, S], the means, the centring
    in place and X @ X.T (BLAS, on the CPUs the process may use).
(a) and (b) alternate --reps times in one process; their M must agree within the bound
derived in tests/correlation_ref.py (8 S 2^-53 sqrt(M_kk M_ll): two float64 results).  The
achieved fp64 multiply-add rate counts the cols^2 S multiply-adds of the full matrix and,
separately, the ones the tile pairs of the upper triangle really do; --fp64-fma-per-s takes
what tools/fp64peak.hip gives on the same box, for orientation only (that is the vector rate,
not the matrix instruction's).  --only-a runs route (a) alone (for a kernel trace).  --out FILE
appends the JSON line to FILE as well as printing it."""

import argparse
import contextlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mcmc-for-nested-data_amd"))

import numpy  # noqa: E402

from nestmc import data  # noqa: E402
from nestmc.engine import Engine  # noqa: E402
from nestmc.families import LinearRegression  # noqa: E402

SHAPES = {"cfg3": (256, 64, 200), "cfg4": (1024, 256, 200)}
TILE = 64                      # NMC_CM_TILE of csrc/comoment.h


def host_comoments(raw):
    rows, cols, C = raw.shape
    X = numpy.ascontiguousarray(numpy.transpose(raw, (1, 0, 2))).reshape(cols, rows * C)
    mean = X.mean(axis=1)
    X -= mean[:, None]
    return mean, X @ X.T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES), default="cfg3")
    ap.add_argument("--chains", type=int, default=0)
    ap.add_argument("--groups", type=int, default=0)
    ap.add_argument("--rows", type=int, default=0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only-a", action="store_true")
    ap.add_argument("--fp64-fma-per-s", type=float, default=0.0)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    C, G, R = SHAPES[a.shape]
    C, G, R = a.chains or C, a.groups or G, a.rows or R
    P, N_obs = 2, 4
    x, y, _, _ = data.linreg(G, N_obs, seed=7)
    fam = LinearRegression.simple(x, y, sigma=1.0)
    eng = Engine(fam, [N_obs] * G, C, "partial", None, seed=1)
    eng.set_schedule(R, 0, 1)                      # R recorded rows; no run()
    cols = eng.cols
    assert eng.n_rows == R and cols == P * (G + 2)
    r = numpy.random.RandomState(0)
    k = numpy.arange(cols)
    scale = 10.0 ** ((k % 5) - 2)
    batch = max(1, (1 << 25) // (cols * C))        # rows written at a time (256 MB)
    for r0 in range(0, R, batch):
        n = min(batch, R - r0)
        z = r.normal(size=(n, cols, C))
        z[:, 1::7] += 0.8 * z[:, 0::7][:, :len(range(1, cols, 7))]       # some correlated pairs
        eng.set_samples_raw((z + 100.0 * (k % 7)[None, :, None]) * scale[None, :, None], r0)
    S = R * C

    def route_b():
        t0 = time.perf_counter()
        raw = eng.samples_raw()
        t1 = time.perf_counter()
        mean, M = host_comoments(raw)
        return (mean, M), time.perf_counter() - t0, t1 - t0

    dev = eng.comoments()                          # warm up
    a_wall, a_kernel, b_wall, b_copy = [], [], [], []
    host = None
    for _ in range(a.reps):
        t0 = time.perf_counter()
        dev = eng.comoments()
        a_wall.append(time.perf_counter() - t0)
        a_kernel.append(eng.event_elapsed_ms(2, 3) * 1e-3)
        if not a.only_a:
            host, w, c = route_b()
            b_wall.append(w)
            b_copy.append(c)
    eng.close()

    m = lambda v: float(numpy.median(v))   # noqa: E731
    nt = (cols + TILE - 1) // TILE
    fma_full = float(cols) * cols * S
    fma_done = float(nt * (nt + 1) // 2) * TILE * TILE * S
    out = {
        "tool": "corrbench", "shape": {"name": a.shape, "chains": C, "groups": G, "rows": R,
                                       "columns": cols, "samples": S},
        "cpus": len(os.sched_getaffinity(0)), "omp_num_threads": os.environ.get("OMP_NUM_THREADS"),
        "a_wall_s": a_wall, "a_kernel_s_events": a_kernel,
        "a_fma_per_s_full_matrix": fma_full / m(a_kernel),
        "a_fma_per_s_tiles_done": fma_done / m(a_kernel),
        "a_bytes_to_host": 8.0 * (cols * cols + 4 * cols),
        "nonfinite": int(dev["nonfinite"].sum()),
    }
    if a.fp64_fma_per_s:
        out["fp64peak_vector_fma_per_s"] = a.fp64_fma_per_s
        out["a_tiles_done_over_fp64peak_vector"] = out["a_fma_per_s_tiles_done"] / a.fp64_fma_per_s
    ok = None
    if host is not None:
        dg = numpy.diagonal(host[1])
        bound = 8.0 * S * 2.0 ** -53 * numpy.sqrt(dg[:, None] * dg[None, :])
        ratio = float((numpy.abs(dev["M"] - host[1]) / bound).max())
        ok = bool(ratio <= 1.0)
        out.update({
            "b_wall_s": b_wall, "b_copy_to_host_s": b_copy, "b_bytes_to_host": 8.0 * cols * S,
            "b_route": "samples_raw + transpose copy + centring + X @ X.T (numpy)",
            "wall_b_over_a": m(b_wall) / m(a_wall),
            "a_spread_s": max(a_wall) - min(a_wall), "b_spread_s": max(b_wall) - min(b_wall),
            "a_vs_b_error_over_bound": ratio, "a_faster_than_b": bool(m(a_wall) < m(b_wall)),
        })
    line = json.dumps(out)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")
    with contextlib.suppress(BrokenPipeError):
        print(line)
    if ok is False:
        sys.exit("device and host comoments differ by more than the bound")


if __name__ == "__main__":
    main()
