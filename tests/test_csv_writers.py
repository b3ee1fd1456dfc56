"""CPU: the CSV writers of csrc/nestmc.hip (put_f, nmc_write_sample_csv, nmc_write_ll_csv) against
Python's own "%f", byte for byte, on the values where fixed formatting goes wrong -- halfway
cases, carries into the next digit or the integer part, signed zeros and NaNs, the smallest
denormal, the largest finite double (316 characters), the infinities -- and on their failure
paths: every fwrite and fclose is checked, so a path that cannot be opened or a full disk
returns -3 with the path in nmc_last_error.  The functions are host code; the library loads
without a GPU.  (nmc_write_ll_csvs needs an engine: tests/test_gpu_outputs.py.)
"""

import ctypes
import os
import struct

import numpy
import pytest


@pytest.fixture(scope="module")
def lib():
    from nestmc import _lib
    return _lib.load()


def _dp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _ip(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))


NEG_NAN = struct.unpack("<d", struct.pack("<Q", 0xFFF8000000000000))[0]
POS_NAN = struct.unpack("<d", struct.pack("<Q", 0x7FF8000000000000))[0]
EDGES = [0.0, -0.0, 5e-324, -5e-324,
         4.9999999e-7, 5e-7, 1.5e-6, 2.5e-6, -4.9999999e-7, -5e-7, -1.5e-6, -2.5e-6,
         0.9999995, 9.9999995, 999999.9999995, -0.9999995, -9.9999995, -999999.9999995,
         2.0 ** 53, 1e15 + 0.5, 1e22, 1e23, -2.0 ** 53, -(1e15 + 0.5), -1e22, -1e23,
         1.7976931348623157e308, -1.7976931348623157e308,
         numpy.inf, -numpy.inf, POS_NAN, NEG_NAN,
         0.5, 1.0, -1.0, 0.1234565, 0.1234575, 123456.7890125, 2.0 ** -1022, 1e-7, 9.9999999e-7]


def _values():
    """The edge values and 2 000 seeded m 10^e, e in [-8, 300], either sign."""
    r = numpy.random.RandomState(4242)
    mant = r.uniform(1.0, 10.0, size=2000) * numpy.where(r.randint(0, 2, size=2000) == 1, 1.0, -1.0)
    e = r.randint(-8, 301, size=2000)
    with numpy.errstate(over="ignore"):
        v = numpy.array([float("%.17ge%d" % (a, b)) for a, b in zip(mant, e)])
    assert numpy.all(numpy.isfinite(v)) and e.min() == -8 and e.max() == 300
    return numpy.concatenate([numpy.array(EDGES), v])


VALUES = _values()


def test_the_edge_values_are_what_they_claim():
    assert numpy.signbit(NEG_NAN) and not numpy.signbit(POS_NAN)
    assert numpy.isnan(NEG_NAN) and numpy.isnan(POS_NAN)
    assert "%f" % NEG_NAN == "nan" and "%f" % POS_NAN == "nan"
    assert "%f" % -0.0 == "-0.000000" and "%f" % 5e-324 == "0.000000"
    assert "%f" % -5e-324 == "-0.000000"
    assert len("%f" % -1.7976931348623157e308) == 317 and len("%f" % 1.7976931348623157e308) == 316
    assert "%f" % 0.9999995 in ("0.999999", "1.000000")         # a carry or not: the double decides
    assert "%f" % 5e-7 in ("0.000000", "0.000001")
    assert "%f" % numpy.inf == "inf" and "%f" % -numpy.inf == "-inf"
    assert len(VALUES) == len(EDGES) + 2000


def _store(cols, C=3):
    """[rows][cols][C]: chain 0 holds VALUES in order, chain 2 holds them reversed, chain 1 a
    value that must never be printed."""
    n = len(VALUES)
    rows = (n + cols - 1) // cols
    pad = numpy.resize(VALUES, rows * cols)
    st = numpy.full((rows, cols, C), 31337.0)
    st[:, :, 0] = pad.reshape(rows, cols)
    st[:, :, 2] = pad[::-1].reshape(rows, cols)
    return numpy.ascontiguousarray(st)


def _index(rows):
    idx = numpy.arange(rows, dtype=numpy.int64) * 3
    idx[:3] = [0, 7, 2 ** 31 - 1]
    idx[-1] = 2 ** 31 - 1
    return numpy.ascontiguousarray(idx, dtype=numpy.int32)


def _sample_text(st, c, idx, chain, n_rows=None):
    n_rows = st.shape[0] if n_rows is None else n_rows
    return "".join("%d,%d," % (idx[r], chain) + ",".join("%f" % v for v in st[r, :, c]) + "\n"
                   for r in range(n_rows))


@pytest.mark.parametrize("cols", [1, 9])
@pytest.mark.parametrize("c", [0, 2])
def test_sample_csv_equals_python_percent_f(lib, tmp_path, cols, c):
    st = _store(cols)
    rows = st.shape[0]
    idx = _index(rows)
    path = str(tmp_path / "s.csv").encode()
    header = "index,chain," + ",".join("p%d" % k for k in range(cols))
    body = _sample_text(st, c, idx, 12)
    assert "31337" not in body

    def call(append, hdr, n_rows=rows, chain=12):
        return lib.nmc_write_sample_csv(path, append, hdr, _dp(st), 3, c, cols, _ip(idx), n_rows,
                                        chain)

    assert call(0, header.encode()) == 0
    want = header + "\n" + body
    got = open(path, "rb").read()
    if got != want.encode():
        gl, wl = got.decode().split("\n"), want.split("\n")
        bad = [i for i in range(min(len(gl), len(wl))) if gl[i] != wl[i]][:3]
        raise AssertionError((cols, c, bad, [(gl[i][:200], wl[i][:200]) for i in bad]))
    # append 1 after append 0, no header; another chain id
    assert call(1, None, chain=0) == 0
    assert open(path, "rb").read() == (want + _sample_text(st, c, idx, 0)).encode()
    # no rows: the header alone is appended, or nothing at all
    assert call(1, b"again", n_rows=0) == 0
    assert call(1, None, n_rows=0) == 0
    assert open(path, "rb").read() == (want + _sample_text(st, c, idx, 0) + "again\n").encode()
    # append 0 truncates; header NULL writes none
    assert call(0, None, n_rows=4) == 0
    assert open(path, "rb").read() == _sample_text(st, c, idx, 12, 4).encode()
    assert call(0, None, n_rows=0) == 0
    assert open(path, "rb").read() == b""


@pytest.mark.parametrize("n", [1, 9])
def test_ll_csv_equals_python_percent_f(lib, tmp_path, n):
    rows = (len(VALUES) + n - 1) // n
    ll = numpy.ascontiguousarray(numpy.resize(VALUES, rows * n).reshape(rows, n))
    path = str(tmp_path / "ll.csv").encode()
    text = "".join(",".join("%f" % v for v in ll[r]) + "\n" for r in range(rows))
    assert lib.nmc_write_ll_csv(path, 0, _dp(ll), n, rows) == 0
    assert open(path, "rb").read() == text.encode()
    assert lib.nmc_write_ll_csv(path, 1, _dp(ll), n, 3) == 0
    assert lib.nmc_write_ll_csv(path, 1, _dp(ll), n, 0) == 0
    first3 = "".join(",".join("%f" % v for v in ll[r]) + "\n" for r in range(3))
    assert open(path, "rb").read() == (text + first3).encode()
    assert lib.nmc_write_ll_csv(path, 0, _dp(ll), n, 0) == 0
    assert open(path, "rb").read() == b""


def _big_ll():
    """60 rows of 1 000 values +-1e300: 309 bytes a value, 18.5 MB of text, so the 16 MiB flush
    of nmc_write_ll_csv is taken (after row 55) and a tail follows it."""
    r = numpy.random.RandomState(77)
    ll = numpy.where(r.randint(0, 2, size=(60, 1000)) == 1, 1e300, -1e300)
    pos, neg = "%f" % 1e300, "%f" % -1e300
    text = "".join(",".join(pos if v > 0 else neg for v in row) + "\n" for row in ll)
    assert len(text) > (1 << 24) + 3 * 309000 and len(pos) == 308
    return numpy.ascontiguousarray(ll), text


def test_ll_csv_flush_branch_byte_identical(lib, tmp_path):
    ll, text = _big_ll()
    path = str(tmp_path / "big.csv").encode()
    assert lib.nmc_write_ll_csv(path, 0, _dp(ll), 1000, 60) == 0
    assert open(path, "rb").read() == text.encode()


def test_writers_report_failure(lib, tmp_path):
    st = _store(9)
    idx = _index(st.shape[0])
    missing = str(tmp_path / "no_such_dir" / "x.csv").encode()
    assert lib.nmc_write_sample_csv(missing, 0, b"h", _dp(st), 3, 0, 9, _ip(idx), 5, 1) == -3
    assert b"no_such_dir" in lib.nmc_last_error()
    assert lib.nmc_write_ll_csv(missing, 0, _dp(st), 9, 5) == -3
    assert b"no_such_dir" in lib.nmc_last_error()
    assert not os.path.exists(str(tmp_path / "no_such_dir"))
    full = "/dev/full"
    writable = False
    if os.path.exists(full):
        try:
            with open(full, "wb", buffering=0) as f:
                f.write(b"x")
        except OSError as e:
            writable = e.errno == 28          # ENOSPC: the device behaves as a full disk
    if not writable:
        print("SKIPPED ASSERTION: no /dev/full that can be opened for writing and is full here; "
              "the short-write returns of the writers were not exercised")
        return
    fb = full.encode()
    assert lib.nmc_write_sample_csv(fb, 0, b"h", _dp(st), 3, 0, 9, _ip(idx), 5, 1) == -3
    assert b"/dev/full" in lib.nmc_last_error()
    assert lib.nmc_write_sample_csv(fb, 1, None, _dp(st), 3, 2, 9, _ip(idx), st.shape[0], 1) == -3
    assert lib.nmc_write_ll_csv(fb, 0, _dp(st), 9, 5) == -3
    assert b"/dev/full" in lib.nmc_last_error()
    ll, _ = _big_ll()                         # the intermediate flush is the write that fails
    assert lib.nmc_write_ll_csv(fb, 1, _dp(ll), 1000, 60) == -3
    assert b"/dev/full" in lib.nmc_last_error()
