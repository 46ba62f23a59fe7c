"""CPU: the host side of the arithmetic family (libvips_amd/csrc/ops_arith.cpp) against the compiled reference -- the
format, band and size decisions of two-image operations over all format pairs, vips_linear's output header, its
single-element rule and its vector-length errors, the avg / sd / row-0 expressions of vips_stats from given sums -- and
the module's classes handing a complex image to the original where no GPU is present."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from libvips_amd import Image, _ffi
from tests import helpers
from tests.helpers import Ref

pytestmark = pytest.mark.skipif(not helpers.have_ref(), reason="oracle/_ref not built")

lib = _ffi.lib
INTERP = helpers.INTERP
VIPS = os.path.join(helpers.ROOT, "oracle", "_ref", "bin", "vips")
OPS = {"add": 3, "subtract": 4, "multiply": 5, "divide": 6}
REAL = [np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32, np.float32, np.float64]


def plan(op, a, b):
    """vips_hip_binary_plan of two (array, interpretation): (format, out_format, bands, interpretation, width, height)."""
    out = [ctypes.c_int() for _ in range(6)]
    args = []
    for array, interp in (a, b):
        h, w, bands = array.shape
        args += [w, h, bands, helpers.DTYPE_FORMATS[array.dtype], interp]
    lib.vips_hip_error_clear()
    if lib.vips_hip_binary_plan(OPS[op], *args, *[ctypes.byref(v) for v in out]) != 0:
        message = _ffi.error_buffer().strip()
        lib.vips_hip_error_clear()
        raise RuntimeError(message)
    return tuple(v.value for v in out)


def ref_header(tmp_path, op, a, b):
    """(format, bands, interpretation, width, height) of `vips <op> a.v b.v out.v`, and the pixels."""
    paths = []
    for i, (array, interp) in enumerate((a, b)):
        paths.append(str(tmp_path / ("in%d.v" % i)))
        helpers.write_v(paths[-1], array, interp)
    out = str(tmp_path / "out.v")
    r = subprocess.run([VIPS, op] + paths + [out], env=helpers.ref_cli_env(), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True)
    if r.returncode != 0:
        raise RuntimeError(r.stderr.strip())
    array, interp = helpers.read_v(out)
    return (helpers.DTYPE_FORMATS[array.dtype], array.shape[2], interp, array.shape[1], array.shape[0]), array


@pytest.mark.parametrize("op", sorted(OPS))
def test_binary_plan_formats(tmp_path, op):
    """Every pair of real formats: the output format is the reference's, and the common format is the one whose
    arithmetic gives the reference's pixels (values that tell the candidates apart: 200 + 100 wraps in no common format
    but is 44 where an operand was clipped to a narrower one)."""
    for ta in REAL:
        for tb in REAL:
            a = (np.array([[[200], [3]]]).astype(ta), INTERP["b-w"])
            b = (np.array([[[100], [2]]]).astype(tb), INTERP["b-w"])
            (fmt, bands, interp, w, h), pixels = ref_header(tmp_path, op, a, b)
            common, out_format, pbands, pinterp, pw, ph = plan(op, a, b)
            assert (out_format, pbands, pinterp, pw, ph) == (fmt, bands, interp, w, h), (op, ta, tb)
            assert out_format == lib.vips_hip_arith_format(OPS[op], common)
            # the reference's pixels are those of the operation done in the common format
            ct = np.dtype(helpers.FORMAT_DTYPES[common])
            lo, hi = (np.iinfo(ct).min, np.iinfo(ct).max) if ct.kind in "ui" else (-np.inf, np.inf)
            x, y = (np.clip(v[0].astype(np.float64), lo, hi) for v in (a, b))  # vips_cast clips
            want = {"add": x + y, "subtract": x - y, "multiply": x * y, "divide": x / y}[op]
            assert np.array_equal(pixels.astype(np.float64), want.astype(helpers.FORMAT_DTYPES[fmt]).astype(np.float64)), (op, ta, tb)


def test_binary_plan_bands_sizes_and_interpretations(tmp_path):
    def im(w, h, bands, interp, dtype=np.uint8):
        return np.ones((h, w, bands), dtype), INTERP[interp]

    cases = [(im(7, 5, 3, "srgb"), im(4, 9, 3, "srgb")), (im(7, 5, 1, "b-w"), im(4, 9, 3, "srgb")),
             (im(7, 5, 3, "srgb"), im(4, 9, 1, "b-w")), (im(3, 3, 3, "multiband"), im(3, 3, 3, "srgb")),
             (im(3, 3, 3, "srgb"), im(3, 3, 3, "multiband")), (im(3, 3, 1, "multiband"), im(3, 3, 4, "srgb", np.uint16)),
             (im(3, 3, 1, "b-w"), im(2, 2, 1, "multiband")), (im(3, 3, 3, "srgb"), im(3, 3, 4, "srgb")),
             (im(3, 3, 4, "srgb"), im(3, 3, 2, "multiband")), (im(3, 3, 2, "multiband"), im(3, 3, 5, "multiband"))]
    for a, b in cases:
        for op in ("add", "divide"):
            try:
                want, _ = ref_header(tmp_path, op, a, b)
            except RuntimeError as e:
                words = str(e).strip().splitlines()[-1]
                with pytest.raises(RuntimeError) as info:
                    plan(op, a, b)
                assert str(info.value) == words, (words, str(info.value))
                continue
            got = plan(op, a, b)
            assert got[1:] == want, (op, a[0].shape, b[0].shape, got, want)


def linear_plan(bands, dtype, a, b, uchar=False):
    args = Image.linear_args(a, b, uchar)
    out_bands, out_format, single = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    ready = [(ctypes.c_double * 32)(), (ctypes.c_double * 32)()]
    lib.vips_hip_error_clear()
    if lib.vips_hip_linear_plan(ctypes.byref(args), bands, helpers.DTYPE_FORMATS[np.dtype(dtype)], ctypes.byref(out_bands),
                                ctypes.byref(out_format), ctypes.byref(single), ready[0], ready[1]) != 0:
        message = _ffi.error_buffer().strip()
        lib.vips_hip_error_clear()
        raise RuntimeError(message)
    return out_bands.value, out_format.value, bool(single.value), list(ready[0]), list(ready[1])


def vec(v):
    return " ".join(repr(float(x)) for x in np.atleast_1d(v))


def test_linear_plan():
    """The output's bands and format, the vector-length errors and the single-element rule for every format: which of
    its two loops the reference took shows in the pixels (1.1 * 107 - 20.3 rounds differently in float and in double)."""
    vectors = [[1.1], [1.1, 1.1], [1.1, 2.5], [1.1, 1.1, 1.1], [1.1, 1.1, 2.5], [1.1, 1.1, 1.1, 1.1]]
    for dtype in REAL:
        for bands in (1, 2, 3):
            src = np.full((1, 2, bands), 107, dtype)
            for a in vectors:
                for b in ([-20.3], [-20.3] * len(a), [-20.3, 7.25, 7.25]):
                    for uchar in (False, True):
                        args = "a=%s,b=%s%s" % (vec(a), vec(b), ",uchar=true" if uchar else "")
                        try:
                            want = Ref.run("linear", src, args)
                        except RuntimeError as e:
                            with pytest.raises(RuntimeError) as info:
                                linear_plan(bands, dtype, a, b, uchar)
                            # (Ref.run puts the operation's name before the reference's own message)
                            assert "linear: " + str(info.value) == str(e).strip().splitlines()[-1], (str(e), str(info.value))
                            continue
                        out_bands, out_format, single, ar, br = linear_plan(bands, dtype, a, b, uchar)
                        assert (out_bands, helpers.FORMAT_DTYPES[out_format]) == (want.shape[2], want.dtype.type), (dtype, bands, a, b)
                        assert single == (len(set(a)) == 1 and len(set(b)) == 1)
                        # a_ready / b_ready (linear.c:181-200)
                        assert ar[:out_bands] == [a[min(k, len(a) - 1)] if len(set(a)) > 1 else a[0] for k in range(out_bands)]
                        assert br[:out_bands] == [b[min(k, len(b) - 1)] if len(set(b)) > 1 else b[0] for k in range(out_bands)]
                        if uchar or want.dtype != np.float32:
                            continue
                        k = np.arange(out_bands)
                        x = np.float32(107)
                        loop1 = np.float32(ar[0]) * x + np.float32(br[0])
                        loopn = (np.asarray(ar)[k] * np.float64(x) + np.asarray(br)[k]).astype(np.float32)
                        assert np.array_equal(want[0, 0], np.full(out_bands, loop1, np.float32) if single else loopn), (dtype, bands, a, b)
    assert np.float32(1.1) * np.float32(107) + np.float32(-20.3) != np.float32(1.1 * 107.0 + -20.3)
    for op in range(7):
        for fmt in (7, 9, -1, 10):
            assert lib.vips_hip_arith_format(op, fmt) == -1
    with pytest.raises(RuntimeError, match="image must be non-complex"):
        linear_plan(1, np.complex64, [1], [0])


@pytest.mark.parametrize("dtype", [np.uint8, np.int8, np.uint16, np.int16, np.float32], ids=lambda d: np.dtype(d).name)
def test_stats_finish(dtype):
    """Rows 1 .. bands of the reference's matrix in, the whole matrix out: row 0's merge, avg and sd are its
    expressions.  (One thread: the reference's choice among equal extremes is then the first in raster order too.)"""
    rng = np.random.default_rng(5)
    for w, h, bands in ((1, 1, 1), (1, 1, 3), (7, 5, 1), (7, 5, 4), (300, 40, 3), (65, 33, 5)):
        src = rng.integers(-100 if np.dtype(dtype).kind != "u" else 0, 120, (h, w, bands)).astype(dtype)
        want = Ref.run("stats", src)[:, :, 0]
        got = want.copy()
        got[0] = -1.0
        got[:, 4:6] = -1.0
        assert lib.vips_hip_stats_finish(got.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), bands, w * h) == 0
        assert np.array_equal(got[:, :6].view(np.uint64), want[:, :6].view(np.uint64)), (w, h, bands, got, want)
        # row 0's positions: those of the band that holds the extreme, the first such band among equals
        k = int(np.argmin(want[1:, 0])), int(np.argmax(want[1:, 1]))
        assert got[0, 6:8].tolist() == want[1 + k[0], 6:8].tolist() and got[0, 8:10].tolist() == want[1 + k[1], 8:10].tolist()
    assert lib.vips_hip_stats_finish(None, 1, 1) != 0
    lib.vips_hip_error_clear()


@pytest.mark.skipif(not helpers.have_module(), reason="host/_build missing")
def test_module_complex_is_the_originals():
    """A complex image never reaches the device: linear_hip, invert_hip and abs_hip hand it to the built-in operation
    (also on a box without a GPU)."""
    Ref.load_module()
    rng = np.random.default_rng(7)
    z = (rng.random((7, 9, 2)) + 1j * rng.random((7, 9, 2))).astype(np.complex64)
    for nick, args in (("linear", "a=2,b=1"), ("linear", "a=2 3,b=1"), ("invert", ""), ("abs", "")):
        got, want = Ref.run(nick + "_hip", z, args), Ref.run(nick, z, args)
        assert got.dtype == want.dtype and np.array_equal(got, want), nick
