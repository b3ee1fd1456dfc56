"""nmc_k_group_order (csrc/grouporder.h) against nestmc.groupcmp's numpy route.

Every result is an integer count, so every comparison is numpy.array_equal: no tolerances.
The shapes sit at the kernel's tiling edges -- the 8 groups of a wave (G = 8, 9), the 64 lanes
of an h chunk (63, 64, 65, 129, 257, 513), the waves of a workgroup by LDS (4 up to G = 640,
2 up to 1280, 1 up to 2560, beyond that the form without LDS), a partial chain block, row
slices (more than 8 rows) -- not at workload size."""

import ctypes
import os

import numpy
import pytest

from gpu_cases import synthetic
from nestmc import _lib
from nestmc import groupcmp as gc
from nestmc.engine import Engine

pytestmark = pytest.mark.gpu

U32 = ctypes.POINTER(ctypes.c_uint32)
I64 = ctypes.POINTER(ctypes.c_int64)
SENT32, SENT64 = 0xDEADBEEF, -7777


def outputs(P, G):
    return (numpy.full((P, G, G), SENT32, dtype=numpy.uint32),
            numpy.full((P, G, G), SENT32, dtype=numpy.uint32),
            numpy.full(P, SENT64, dtype=numpy.int64))


def untouched(h, w, b):
    return bool((h == SENT32).all() and (w == SENT32).all() and (b == SENT64).all())


def go_of(lib, x, P, G, partial, n_valid, rows=None, C=None):
    h, w, b = outputs(P, G)
    rc = lib.nmc_group_order_of(0, _lib.dptr(x), x.shape[0] if rows is None else rows, P, G,
                                int(partial), x.shape[2] if C is None else C, n_valid,
                                h.ctypes.data_as(U32), w.ctypes.data_as(U32),
                                b.ctypes.data_as(I64))
    return rc, h, w, b


def same(h, w, b, want):
    assert numpy.array_equal(h, want["hist"]), "hist"
    assert numpy.array_equal(w, want["wins"]), "wins"
    assert numpy.array_equal(b, want["nonfinite"]), "nonfinite"


def invariants(h, w, S):
    h, w = h.astype(numpy.int64), w.astype(numpy.int64)
    G = h.shape[1]
    assert (h.sum(axis=2) == S).all()
    assert numpy.array_equal(w.sum(axis=2), (h * numpy.arange(G)).sum(axis=2))
    assert not numpy.diagonal(w, axis1=1, axis2=2).any()
    assert (w + numpy.transpose(w, (0, 2, 1)) <= S).all()


def rand_store(seed, rows, P, G, partial, C):
    r = numpy.random.RandomState(seed)
    return r.normal(size=(rows, P * (G + 2 * partial), C))


# ---- 1. nmc_group_order_of on injected stores -----------------------------------------------
#        (G, rows, C, n_valid, partial, P)
SHAPES = [(2, 1, 1, 1, 0, 2), (3, 5, 64, 64, 1, 2), (8, 1, 66, 65, 0, 2), (9, 5, 130, 129, 1, 2),
          (63, 1, 64, 64, 0, 2), (64, 5, 66, 65, 1, 2), (65, 1, 130, 129, 0, 2),
          (129, 5, 1, 1, 1, 2), (257, 1, 66, 65, 1, 2), (513, 2, 3, 3, 0, 2),
          (5, 5, 66, 65, 1, 3), (5, 1, 64, 64, 0, 3),          # a wrong parameter stride shows
          (9, 19, 66, 65, 1, 2),                               # three row slices: 7, 7, 5 rows
          (32, 3, 3, 2, 0, 1), (33, 3, 3, 2, 1, 1),            # a workgroup's 4 x 8 groups
          (640, 1, 2, 2, 0, 1), (641, 1, 2, 2, 1, 1),          # 4 waves | 2 waves
          (1280, 1, 2, 2, 0, 1), (1281, 1, 2, 1, 0, 1),        # 2 waves | 1 wave
          (2560, 1, 2, 2, 0, 1), (2561, 1, 3, 2, 0, 1)]        # 1 wave | no LDS


@pytest.mark.parametrize("G,rows,C,n_valid,partial,P", SHAPES)
def test_group_order_of(gpu_lib, G, rows, C, n_valid, partial, P):
    x = rand_store(G * 31 + rows, rows, P, G, partial, C)
    if n_valid < C:
        x[:, :, n_valid:] = numpy.nan        # padding chains: never counted
    if partial:
        x[:, ::G + 2] = numpy.inf            # _mu and _sigma2 are no groups
        x[:, 1::G + 2] = -numpy.inf
    rc, h, w, b = go_of(gpu_lib, x, P, G, partial, n_valid)
    assert rc == 0, gpu_lib.nmc_last_error()
    want = gc.counts_from_samples(x, P, G, partial, n_valid)
    same(h, w, b, want)
    assert not b.any()
    invariants(h, w, rows * n_valid)


# ---- 2. ties and signed zeros -------------------------------------------------------------------
def test_ties_and_signed_zeros(gpu_lib):
    r = numpy.random.RandomState(4)
    rows, P, G, C, nv = 6, 2, 70, 66, 65
    x = r.randint(-2, 3, size=(rows, P * (G + 2), C)).astype(numpy.float64)
    x = numpy.where(r.uniform(size=x.shape) < 0.5, x, -x)        # -0.0 against +0.0
    assert numpy.signbit(x[x == 0]).any() and not numpy.signbit(x[x == 0]).all()
    rc, h, w, b = go_of(gpu_lib, x, P, G, 1, nv)
    assert rc == 0
    want = gc.counts_from_samples(x, P, G, True, nv)
    same(h, w, b, want)
    S = rows * nv
    invariants(h, w, S)
    col = gc.group_columns(P, G, True)
    for p in range(P):
        th = x[:, col[p], :nv]
        eq = (th[:, :, None, :] == th[:, None, :, :]).sum(axis=(0, 3))
        assert numpy.array_equal(w[p].astype(numpy.int64) + w[p].T, S - eq)
        assert (eq < S).any() and (eq[~numpy.eye(G, dtype=bool)] > 0).all()


def test_all_equal_store(gpu_lib):
    rows, P, G, C, nv = 3, 2, 67, 66, 66
    x = numpy.full((rows, P * G, C), 1.5)
    x[:, 5] = 1.5
    rc, h, w, b = go_of(gpu_lib, x, P, G, 0, nv)
    assert rc == 0
    assert (h[:, :, 0] == rows * nv).all() and not h[:, :, 1:].any()
    assert not w.any() and not b.any()


# ---- 3. non-finite values -----------------------------------------------------------------------
def nonfinite_store():
    rows, P, G, C = 4, 2, 11, 66
    x = rand_store(9, rows, P, G, 1, C)
    col = gc.group_columns(P, G, True)
    x[0, col[0, 3], 0] = numpy.nan
    x[1, col[0, 10], 64] = numpy.inf
    x[3, col[0, 0], 65] = -numpy.inf
    x[2, col[1, 8], 7] = numpy.nan
    x[2, col[1, 9], 7] = numpy.nan
    x[2, col[1, 2], 7] = numpy.inf
    x[0, col[1, 2], 33] = -numpy.inf
    x[0, 1, 5] = numpy.nan                  # a hyper column: not a group, not counted
    return x, P, G


def test_nonfinite_counts(gpu_lib):
    x, P, G = nonfinite_store()
    rc, h, w, b = go_of(gpu_lib, x, P, G, 1, 66)
    assert rc == 0
    assert b.tolist() == [3, 4]
    same(h, w, b, gc.counts_from_samples(x, P, G, True, 66))
    assert (h.astype(numpy.int64).sum(axis=2) == 4 * 66).all()
    rc, h, w, b = go_of(gpu_lib, x, P, G, 1, 65)            # chain 65 is padding now
    assert rc == 0 and b.tolist() == [2, 4]
    same(h, w, b, gc.counts_from_samples(x, P, G, True, 65))


# ---- 4. bad arguments ---------------------------------------------------------------------------
def test_bad_arguments_of(gpu_lib):
    x = rand_store(1, 2, 1, 4, 1, 3)                          # rows 2, cols 6, C 3
    bad = [dict(n_valid=0), dict(n_valid=4), dict(rows=0), dict(C=0), dict(G=1, P=6),
           dict(partial=2), dict(partial=-1), dict(P=0),
           dict(rows=65536, C=32768, n_valid=32768, G=2, P=1, partial=0)]   # S = 2^31
    for kw in bad:
        a = dict(P=1, G=4, partial=1, n_valid=3, rows=None, C=None)
        a.update(kw)
        rc, h, w, b = go_of(gpu_lib, x, a["P"], a["G"], a["partial"], a["n_valid"], a["rows"],
                            a["C"])
        assert rc == -1, kw
        assert untouched(h, w, b), kw
    # (cols == P (G + 2 partial) is how the array is read: P = 1, G = 4 with partial = 0 reads
    # the first 4 columns of every 4 -- a caller's mistake no call can see; the Python layer
    # checks shapes)
    with pytest.raises(ValueError):
        gc.counts_from_samples(x, 1, 4, False)


def small_engine(C, G=6, chain_base=0, rows=12, pooling="partial"):
    kind = {"partial": "linreg_partial", "none": "regression3_none",
            "complete": "linreg_complete"}[pooling]
    fam, sizes, priors, pooling, names = synthetic(kind, C, G, 8)
    eng = Engine(fam, sizes, C, pooling, priors, seed=2, chain_base=chain_base)
    eng.set_schedule(rows, 0, 1)          # rows recorded rows; no run()
    return eng


def test_bad_arguments_engine(gpu_lib):
    eng = small_engine(5)
    try:
        eng.set_samples_raw(rand_store(2, 12, 2, 6, 1, 5))
        for rb, nr, nv in ((-1, 2, 5), (11, 2, 5), (0, 13, 5), (0, 0, 5), (3, -1, 5), (0, 12, 0),
                           (0, 12, 6)):
            h, w, b = outputs(2, 6)
            rc = eng.lib.nmc_group_order(eng.h, rb, nr, nv, h.ctypes.data_as(U32),
                                         w.ctypes.data_as(U32), b.ctypes.data_as(I64))
            assert rc == -1 and untouched(h, w, b), (rb, nr, nv)
        with pytest.raises(_lib.NestmcError):
            eng.group_order_counts(n_valid=6)
    finally:
        eng.close()
    one = small_engine(3, pooling="complete")                 # one group
    try:
        h, w, b = outputs(3, 1)
        rc = one.lib.nmc_group_order(one.h, 0, 12, 3, h.ctypes.data_as(U32),
                                     w.ctypes.data_as(U32), b.ctypes.data_as(I64))
        assert rc == -1 and untouched(h, w, b)
        assert b"two groups" in one.lib.nmc_last_error()
    finally:
        one.close()


# ---- 5. the Engine path -------------------------------------------------------------------------
def test_engine_row_windows_and_shards(gpu_lib):
    C, G, rows = 130, 6, 12
    x = rand_store(3, rows, 2, G, 1, C)
    x[2:5, 4] = x[2:5, 5]                                       # some exact ties
    eng = small_engine(C)
    try:
        eng.set_samples_raw(x)
        ev0 = eng.group_order_counts()
        assert ev0["n_samples"] == rows * C and ev0["hist"].dtype == numpy.int64
        want = gc.counts_from_samples(x, 2, G, True)
        same(ev0["hist"], ev0["wins"], ev0["nonfinite"], want)
        assert eng.event_elapsed_ms(4, 5) >= 0.0                   # slots 4 / 5 bracket the kernel
        for rb, nr, nv in ((0, 1, C), (5, 7, C), (11, 1, 129), (3, 6, 65), (0, 12, 1)):
            got = eng.group_order_counts(rb, nr, nv)
            w = gc.counts_from_samples(x[rb:rb + nr], 2, G, True, nv)
            same(got["hist"], got["wins"], got["nonfinite"], w)
            assert got["n_samples"] == nr * nv
        res = eng.group_comparison(["b0", "b1"])
        ref = gc.finish(want["hist"], want["wins"], want["n_samples"], ["b0", "b1"])
        for k in ("mean_rank", "median_rank", "rank_lo", "rank_hi", "p_lowest", "p_highest",
                  "p_greater", "hist", "wins"):
            assert numpy.array_equal(getattr(res, k), getattr(ref, k)), k
        assert res.probability_greater("b1", 2, 3) == want["wins"][1, 2, 3] / (rows * C)
    finally:
        eng.close()
    # two engines with chain_base shards: 70 chains (the last block partial) + 60 chains of
    # which 58 count (n_valid < C); merged = one engine over the 128 chains
    a, b = small_engine(70), small_engine(60, chain_base=70)
    try:
        a.set_samples_raw(numpy.ascontiguousarray(x[:, :, :70]))
        b.set_samples_raw(numpy.ascontiguousarray(x[:, :, 70:]))
        parts = [a.group_order_counts(), b.group_order_counts(n_valid=58)]
        m = gc.merge(parts)
        w = gc.counts_from_samples(x, 2, G, True, 128)
        same(m["hist"], m["wins"], m["nonfinite"], w)
        assert m["n_samples"] == rows * 128
    finally:
        a.close()
        b.close()


def test_engine_nonfinite_raises(gpu_lib):
    x, P, G = nonfinite_store()
    eng = small_engine(66, G=G, rows=4)
    try:
        eng.set_samples_raw(x)
        raw = eng.group_order_counts()
        assert raw["nonfinite"].tolist() == [3, 4]
        with pytest.raises(_lib.NestmcError, match="7 group values were not finite"):
            eng.group_comparison()
        assert eng.group_nonfinite == 7
        ok = eng.group_comparison(row_begin=1, n_rows=1, n_valid=64)   # a clean window
        assert ok.n_samples == 64
    finally:
        eng.close()


# ---- 6. sample_posterior(computeGroupComparison=True) ----------------------------------------
def _api_case():
    C, G, N = 66, 6, 20
    fam, sizes, priors, pooling, names = synthetic("linreg_partial", C, G, N)
    kw = dict(saveLogLikelihood=False, priorDistribution=priors,
              startingPointValueRange={n: [-0.5, 0.5] for n in names}, displayProgress=False,
              seed=17, return_samples=True, computeGroupComparison=True)
    return (C, 60, 15, names, G, N, pooling, fam), kw        # burn 30, thin 2: 15 rows


FIELDS = ("hist", "wins", "mean_rank", "median_rank", "rank_lo", "rank_hi", "p_lowest",
          "p_highest", "p_greater")


def _files(d):
    return tuple(open(os.path.join(d, f), "rb").read()
                 for f in (gc.FILE_RANKING, gc.FILE_PAIRWISE))


@pytest.fixture(scope="module")
def one_run(gpu_lib, tmp_path_factory):
    """The one-engine run the other routes are compared with: (result dict, directory)."""
    from nestmc.sampler import sample_posterior
    args, kw = _api_case()
    one_dir = str(tmp_path_factory.mktemp("groupcmp") / "one")
    return sample_posterior(*args, one_dir, **kw), one_dir


def _same_result(got, one, what):
    for k in FIELDS:
        assert numpy.array_equal(getattr(got, k), getattr(one["group_comparison"], k)), (what, k)


def test_sample_posterior_group_comparison(one_run):
    one, one_dir = one_run
    C, G = 66, 6
    res = one["group_comparison"]
    assert sorted(os.listdir(one_dir)) == [gc.FILE_PAIRWISE, gc.FILE_RANKING, "log", "sample"]
    assert one["rows"].shape == (C, 15, 2 * (G + 2)) and res.names == ["b0", "b1"]
    raw = numpy.ascontiguousarray(numpy.transpose(one["rows"], (1, 2, 0)))
    want = gc.counts_from_samples(raw, 2, G, True)
    assert res.n_samples == 15 * C
    assert numpy.array_equal(res.hist, want["hist"])
    assert numpy.array_equal(res.wins, want["wins"])
    rk = open(os.path.join(one_dir, gc.FILE_RANKING)).read().splitlines()
    pw = open(os.path.join(one_dir, gc.FILE_PAIRWISE)).read().splitlines()
    assert rk[0] == gc.HEADER_RANKING and len(rk) == 1 + 2 * G
    assert pw[0] == gc.HEADER_PAIRWISE and len(pw) == 1 + 2 * G * (G - 1)
    back = gc.read_csvs(one_dir)
    for k in FIELDS[1:]:
        assert numpy.array_equal(back[k], getattr(res, k)), k


def test_sample_posterior_two_engines(one_run, tmp_path):
    """devices=[0, 0]: 33 + 33 chains, the counts merged in engine order."""
    from nestmc.sampler import sample_posterior
    one, one_dir = one_run
    args, kw = _api_case()
    two_dir = str(tmp_path / "two")
    two = sample_posterior(*args, two_dir, **dict(kw, devices=[0, 0]))
    assert numpy.array_equal(two["rows"], one["rows"])
    _same_result(two["group_comparison"], one, "two engines")
    assert _files(two_dir) == _files(one_dir)


def test_sample_posterior_chain_halves(one_run, tmp_path):
    """Two chains= shards (40 + 26 chains), merged by the caller."""
    from nestmc.sampler import sample_posterior
    one, one_dir = one_run
    args, kw = _api_case()
    halves = [sample_posterior(*args, None, **dict(kw, write_files=False, chains=ch))
              for ch in (list(range(0, 40)), list(range(40, 66)))]
    m = gc.merge([dict(hist=h["group_comparison"].hist, wins=h["group_comparison"].wins,
                       nonfinite=numpy.zeros(2, dtype=numpy.int64),
                       n_samples=h["group_comparison"].n_samples) for h in halves])
    merged = gc.finish(m["hist"], m["wins"], m["n_samples"], ["b0", "b1"])
    _same_result(merged, one, "chain halves")
    gc.write_csvs(merged, str(tmp_path))
    assert _files(str(tmp_path)) == _files(one_dir)


def test_sample_posterior_process_per_device(one_run, tmp_path):
    """process_per_device: the rank's counts travel over the host group to rank 0."""
    from nestmc.sampler import sample_posterior
    one, one_dir = one_run
    args, kw = _api_case()
    ppd_dir = str(tmp_path / "ppd")
    ppd = sample_posterior(*args, ppd_dir, **dict(kw, devices=[0], process_per_device=True))
    assert numpy.array_equal(ppd["rows"], one["rows"])
    _same_result(ppd["group_comparison"], one, "process_per_device")
    assert _files(ppd_dir) == _files(one_dir)


def test_sample_posterior_default_off_and_complete(gpu_lib, tmp_path):
    from nestmc.sampler import sample_posterior
    args, kw = _api_case()
    off_dir = str(tmp_path / "off")
    off = sample_posterior(*args, off_dir, **dict(kw, computeGroupComparison=False))
    assert sorted(os.listdir(off_dir)) == ["log", "sample"]
    assert sorted(off) == ["accepted", "burn", "header", "loop_seconds", "row_index", "rows",
                           "thin"]
    fam, sizes, priors, pooling, names = synthetic("linreg_complete", 4, 3, 10)
    never = str(tmp_path / "never")
    with pytest.raises(ValueError, match="computeGroupComparison"):
        sample_posterior(4, 20, 5, names, 3, 10, pooling, fam, never, priorDistribution=priors,
                         displayProgress=False, computeGroupComparison=True)
    assert not os.path.exists(never)
