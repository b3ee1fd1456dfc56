#!/usr/bin/env python
"""Group rankings and pairwise comparisons at the cfg-3 and cfg-4 store shapes: two parameters
under partial pooling, 64 groups x 256 chains x 200 recorded rows (S = 51 200 samples, 132
columns) and 256 groups x 1 024 chains x 200 rows (S = 204 800, 516 columns, 845 MB).  The
store is written with nmc_debug_set_samples (group effects plus noise; no sampling).

(a) the device route: Engine.group_order_counts() over the whole store -- host clock around
    the call (allocation and zeroing of the two count arrays, the kernel, their copy) and the
    context's events around the kernel alone (slots 4 / 5, nmc_group_order);
(b) the host route on the same store: Engine.samples_raw() (the copy of the whole store) plus
    nestmc.groupcmp.counts_from_samples, the broadcast-compare formulation in numpy (an
    argsort gives ranks only where no two values tie and gives no pairwise counts, so the
    compare, which both results need, is the host's best single pass).
(a) and (b) alternate --reps times in one process and must agree as integers.  --b-rows K:
route (b) counts the first K rows only and its counting time is EXTRAPOLATED linearly to all
rows (the copy is still the whole store's); parity is then checked on those K rows against
the device's counts of the same row window.  --only-a runs route (a) alone (for a kernel
trace).  --out FILE appends the JSON line to FILE as well as printing it."""

import argparse
import contextlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mcmc-for-nested-data_amd"))

import numpy  # noqa: E402

from nestmc import data, groupcmp  # noqa: E402
from nestmc.engine import Engine  # noqa: E402
from nestmc.families import LinearRegression  # noqa: E402

SHAPES = {"cfg3": (256, 64, 200), "cfg4": (1024, 256, 200)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES), default="cfg3")
    ap.add_argument("--chains", type=int, default=0)
    ap.add_argument("--groups", type=int, default=0)
    ap.add_argument("--rows", type=int, default=0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only-a", action="store_true")
    ap.add_argument("--b-rows", type=int, default=0)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    C, G, R = SHAPES[a.shape]
    C, G, R = a.chains or C, a.groups or G, a.rows or R
    P, N_obs = 2, 4
    x, y, _, _ = data.linreg(G, N_obs, seed=7)
    fam = LinearRegression.simple(x, y, sigma=1.0)
    eng = Engine(fam, [N_obs] * G, C, "partial", None, seed=1)
    eng.set_schedule(R, 0, 1)                      # R recorded rows; no run()
    assert eng.n_rows == R and eng.cols == P * (G + 2)
    r = numpy.random.RandomState(0)
    effect = numpy.zeros(eng.cols)
    effect[groupcmp.group_columns(P, G, True).ravel()] = r.normal(size=P * G)
    batch = max(1, (1 << 25) // (eng.cols * C))    # rows written at a time (256 MB)
    for r0 in range(0, R, batch):
        n = min(batch, R - r0)
        eng.set_samples_raw(effect[None, :, None] + 0.5 * r.normal(size=(n, eng.cols, C)), r0)
    S = R * C
    Rb = a.b_rows if 0 < a.b_rows < R else R

    def route_b():
        t0 = time.perf_counter()
        raw = eng.samples_raw()
        t1 = time.perf_counter()
        host = groupcmp.counts_from_samples(raw[:Rb], P, G, True)
        t2 = time.perf_counter()
        return host, (t1 - t0) + (t2 - t1) * (R / Rb), t1 - t0

    dev = eng.group_order_counts()                 # warm up
    a_wall, a_kernel, b_wall, b_copy = [], [], [], []
    host = None
    for _ in range(a.reps):
        t0 = time.perf_counter()
        dev = eng.group_order_counts()
        a_wall.append(time.perf_counter() - t0)
        a_kernel.append(eng.event_elapsed_ms(4, 5) * 1e-3)
        if not a.only_a:
            host, w, c = route_b()
            b_wall.append(w)
            b_copy.append(c)
    same = None
    if host is not None:
        d = dev if Rb == R else eng.group_order_counts(0, Rb)
        same = bool(all(numpy.array_equal(d[k], host[k]) for k in ("hist", "wins", "nonfinite"))
                    and d["n_samples"] == host["n_samples"])
    res = groupcmp.finish(dev["hist"], dev["wins"], dev["n_samples"])
    eng.close()

    m = lambda v: float(numpy.median(v))   # noqa: E731
    pairs = float(S) * P * G * G
    out = {
        "tool": "groupbench", "shape": {"name": a.shape, "chains": C, "groups": G, "rows": R,
                                        "parameters": P, "samples": S, "pairs": pairs},
        "a_wall_s": a_wall, "a_kernel_s_events": a_kernel,
        "a_pairs_per_s_kernel": pairs / m(a_kernel),
        # ~2 fp64-rate instructions per pair per wave of 64 pairs, 1 024 SIMDs at 2.4 GHz, 4
        # cycles per wave instruction (16 fp64 lanes per SIMD and clock)
        "floor_s_instruction_count": pairs / 64 * 2 * 4 / (1024 * 2.4e9),
        "a_bytes_to_host": 4.0 * 2 * P * G * G + 8 * P,
        "nonfinite": int(dev["nonfinite"].sum()),
        "mean_rank_span": [float(res.mean_rank.min()), float(res.mean_rank.max())],
    }
    out["a_kernel_over_floor"] = m(a_kernel) / out["floor_s_instruction_count"]
    if host is not None:
        out.update({
            "b_rows_timed": Rb, "b_wall_extrapolated": bool(Rb < R), "b_wall_s": b_wall,
            "b_copy_to_host_s": b_copy, "b_bytes_to_host": 8.0 * eng.cols * S,
            "b_route": "samples_raw + groupcmp.counts_from_samples (broadcast compare)",
            "wall_b_over_a": m(b_wall) / m(a_wall),
            "a_spread_s": max(a_wall) - min(a_wall), "b_spread_s": max(b_wall) - min(b_wall),
            "same_integers": same,
        })
    line = json.dumps(out)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")
    with contextlib.suppress(BrokenPipeError):
        print(line)
    if same is False:
        sys.exit("device and host counts differ")


if __name__ == "__main__":
    main()
