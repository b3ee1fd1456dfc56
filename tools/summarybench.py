#!/usr/bin/env python
"""Median and HDI of every column at the cfg-3 store shape: 256 chains x 132 columns (64
groups, two parameters, partial pooling) x 200 recorded rows, N = 51 200 values per column.

(a) the device route: Engine.summary() over the whole store -- host clock around the call (the
    allocation of the key buffers, the sort and scan kernels, the copy of the per-column
    results, finish on the host) and the context's events around the kernels alone (slots
    10 / 11, nmc_summary);
(b) the only route without the sort kernels, on the same store: Engine.samples_raw() ->
    numpy.sort, numpy.median and nestmc.diagnosis.hpd_interval per column.
(a) and (b) alternate --reps times in one process.  Parity: every statistic of (a) equals (b)
bit for bit.  Bytes and passes come from the shapes (csrc/sortcol.h): the tile sort reads the
window and writes K N keys, every merge pass and the scan read and/or write K N keys.  Prints
one JSON line."""

import argparse
import contextlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mcmc-for-nested-data_amd"))

import numpy  # noqa: E402

from nestmc import data, diagnosis  # noqa: E402
from nestmc.engine import Engine  # noqa: E402
from nestmc.families import LinearRegression  # noqa: E402

TILE = 4096                      # csrc/sortcol.h NMC_SORT_TILE
HBM_PEAK_BYTES_PER_S = 8.0e12    # MI355X HBM3E


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=256)
    ap.add_argument("--groups", type=int, default=64)
    ap.add_argument("--obs", type=int, default=100)
    ap.add_argument("--rows", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    C, G, N_obs, R = a.chains, a.groups, a.obs, a.rows
    x, y, _, _ = data.linreg(G, N_obs, seed=7)
    fam = LinearRegression.simple(x, y, sigma=1.0)
    eng = Engine(fam, [N_obs] * G, C, "partial", None, seed=1)
    r = numpy.random.RandomState(0)
    value = numpy.array([0.0, 2.0])[None, :, None] + 0.1 * r.normal(size=(C, 2, G))
    eng.set_state(value, numpy.zeros((C, 2, G)), eng.eval_group_ll(value),
                  numpy.tile([0.0, 2.0], (C, 1)), numpy.full((C, 2), 0.5))
    eng.set_schedule(2 * R, R, 1)
    eng.run(0, 2 * R)
    eng.synchronize()
    assert eng.n_rows == R
    K, N = eng.cols, R * C

    def route_b():
        t0 = time.perf_counter()
        raw = eng.samples_raw()                                   # [rows][cols][C]
        t1 = time.perf_counter()
        flat = numpy.ascontiguousarray(numpy.transpose(raw, (1, 0, 2))).reshape(K, N)
        med = numpy.array([numpy.median(c) for c in flat])
        hdi = numpy.array([diagnosis.hpd_interval(c, 95) for c in flat])
        return med, hdi, time.perf_counter() - t0, t1 - t0

    eng.summary()                                # warm up
    route_b()
    a_wall, a_kernel, b_wall, b_copy = [], [], [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        res = eng.summary()
        a_wall.append(time.perf_counter() - t0)
        a_kernel.append(eng.event_elapsed_ms(10, 11) * 1e-3)
        med, hdi, w, c = route_b()
        b_wall.append(w)
        b_copy.append(c)
    eng.close()

    w64 = lambda v: numpy.ascontiguousarray(v, dtype=numpy.float64).view(numpy.uint64)  # noqa: E731
    same = bool(numpy.array_equal(w64(res.median), w64(med))
                and numpy.array_equal(w64(res.hdi_lower), w64(hdi[:, 0]))
                and numpy.array_equal(w64(res.hdi_upper), w64(hdi[:, 1])))
    tiles = (N + TILE - 1) // TILE
    passes = 0
    while (TILE << passes) < N:
        passes += 1
    kn8 = 8.0 * K * N
    # tile sort: reads the window, writes the keys; a merge pass: reads and writes them; the
    # scan reads them about twice (s[i] and s[i + gap])
    kernel_bytes = 2 * kn8 * (1 + passes) + 2 * kn8
    m = lambda v: float(numpy.median(v))   # noqa: E731
    out = {
        "shape": {"chains": C, "columns": K, "rows": R, "values_per_column": N, "tiles": tiles},
        "a_wall_s": a_wall, "a_kernels_s_events": a_kernel,
        "b_wall_s": b_wall, "b_copy_to_host_s": b_copy,
        "wall_a_over_b": m(a_wall) / m(b_wall),
        "a_faster_than_b": bool(m(a_wall) < m(b_wall)),
        "merge_passes": passes, "bytes_per_pass_read_plus_written": 2 * kn8,
        "kernel_bytes_total": kernel_bytes,
        "kernel_bytes_per_s": kernel_bytes / m(a_kernel),
        "kernel_share_of_hbm_peak": kernel_bytes / m(a_kernel) / HBM_PEAK_BYTES_PER_S,
        "b_bytes_to_host": kn8, "a_bytes_to_host": 8.0 * K * 8,
        "parity_bit_identical": same,
    }
    with contextlib.suppress(BrokenPipeError):
        print(json.dumps(out))


if __name__ == "__main__":
    main()
