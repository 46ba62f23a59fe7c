"""CPU: the host side of vips_spcor (libvips_amd/csrc/ops_correlation.cpp): the per-band constants of
vips_spcor_pre_generate (spcor.c:99-152) against a numpy restatement of vips_avg, vips_linear (both of its loops),
vips_multiply and vips_avg again, and the refusals of the ABI that need no device.  No device is touched."""
import ctypes

import numpy as np
import pytest

from libvips_amd import _ffi
from tests import helpers

lib = _ffi.lib
DTYPES = [np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32, np.float32, np.float64]
name_of = lambda d: np.dtype(d).name  # noqa: E731


def raster_sum(values):
    """A double sum in raster order (np.sum adds pairwise)."""
    total = np.float64(0.0)
    for v in np.asarray(values, np.float64).ravel():
        total = total + v
    return total


def model(ref, out_bands):
    """-> (rmean, c1) of a ref after format matching, its one band replicated to out_bands."""
    h, w, bands = ref.shape
    pick = lambda b: ref[:, :, 0 if bands == 1 else b]  # noqa: E731
    n = np.float64(w * h)
    rmean = [raster_sum(pick(b)) / n for b in range(out_bands)]
    single = all(m == rmean[0] for m in rmean)  # linear.c:155-179
    c1 = []
    for b in range(out_bands):
        band = pick(b)
        if ref.dtype == np.float64:
            sq = (np.float64(1.0) * band + (-rmean[b])) ** 2  # linear, multiply and avg stay double
        else:
            p = band.astype(np.float32)
            if single:
                v = np.float32(1.0) * p + np.float32(-rmean[0])  # LOOP1: float constants, float arithmetic
                assert v.dtype == np.float32
            else:
                v = (np.float64(1.0) * p.astype(np.float64) + (-rmean[b])).astype(np.float32)  # LOOPN: double, rounded
            sq = v * v
            assert sq.dtype == np.float32
        c1.append(np.sqrt((raster_sum(sq) / n) * n))
    return np.array(rmean), np.array(c1)


def constants(ref, out_bands, stride=None):
    h, w, bands = ref.shape
    row = w * bands * ref.dtype.itemsize
    stride = stride or row
    buf = np.zeros(h * stride, np.uint8)
    for y in range(h):
        buf[y * stride:y * stride + row] = np.ascontiguousarray(ref[y]).view(np.uint8).ravel()
    rmean, c1 = (ctypes.c_double * out_bands)(), (ctypes.c_double * out_bands)()
    rc = lib.vips_hip_spcor_constants(buf.ctypes.data, w, h, bands, helpers.DTYPE_FORMATS[ref.dtype], stride, out_bands, rmean, c1)
    assert rc == 0, _ffi.error_buffer()
    return np.array(rmean), np.array(c1)


def noise(w, h, bands, dtype, seed):
    rng = np.random.default_rng(seed)
    dt = np.dtype(dtype)
    if dt.kind in "ui":
        info = np.iinfo(dt)
        return rng.integers(info.min, info.max, (h, w, bands), dtype=dt, endpoint=True)
    return ((rng.random((h, w, bands)) - 0.5) * 600.0).astype(dt)


def bits(a):
    return np.asarray(a, np.float64).view(np.uint64)


@pytest.mark.parametrize("dtype", DTYPES, ids=name_of)
def test_constants_vector_loop(dtype):
    """Three bands of differing means: vips_linear's vector loop; rows with padding behind them."""
    ref = noise(8, 7, 3, dtype, 3)
    want = model(ref, 3)
    assert len(set(want[0])) == 3
    for stride in (None, 8 * 3 * ref.dtype.itemsize + 16):
        got = constants(ref, 3, stride)
        assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(want[1])), (got, want)


@pytest.mark.parametrize("dtype", DTYPES, ids=name_of)
def test_constants_single_loop(dtype):
    """One band, one band replicated to three, and three bands of equal means: the single-constant loop."""
    one = noise(17, 16, 1, dtype, 5)
    for out_bands in (1, 3):
        got, want = constants(one, out_bands), model(one, out_bands)
        assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(want[1])), (got, want)
    three = noise(8, 7, 3, dtype, 7)
    if np.dtype(dtype).kind == "f":
        three = np.round(three)
    three[:, :, 1] = three[::-1, ::-1, 0]
    three[:, :, 2] = np.roll(three[:, :, 0], 3, axis=1)
    got, want = constants(three, 3), model(three, 3)
    assert want[0][0] == want[0][1] == want[0][2]
    assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(want[1])), (got, want)


def test_the_two_loops_differ():
    """The float rounding of -rmean shows: the same band gives another c1 beside a band of another mean."""
    ref = noise(8, 7, 1, np.uint8, 9)
    alone = constants(ref, 1)[1][0]
    other = np.concatenate([ref, (ref // 2)], axis=2)
    beside = constants(other, 2)[1][0]
    assert alone == model(ref, 1)[1][0] and beside == model(other, 2)[1][0]
    assert alone != beside


def test_constant_ref():
    rmean, c1 = constants(np.full((4, 5, 2), 77, np.uint8), 2)
    assert list(rmean) == [77.0, 77.0] and list(c1) == [0.0, 0.0]


def test_constants_refusals():
    buf = np.zeros(64, np.uint8)
    out = (ctypes.c_double * 4)()
    cases = [
        ((None, 4, 4, 1, 0, 4, 1, out, out), "spcor: bad arguments"),
        ((buf.ctypes.data, 0, 4, 1, 0, 4, 1, out, out), "spcor: bad arguments"),
        ((buf.ctypes.data, 4, 4, 1, 0, 4, 1, None, out), "spcor: bad arguments"),
        ((buf.ctypes.data, 2, 2, 1, 7, 16, 1, out, out), "spcor: image must be non-complex"),
        ((buf.ctypes.data, 2, 2, 1, 42, 16, 1, out, out), "spcor: unknown band format 42"),
        ((buf.ctypes.data, 2, 2, 3, 0, 6, 4, out, out), "spcor: not one band or 4 bands"),
    ]
    for args, words in cases:
        lib.vips_hip_error_clear()
        assert lib.vips_hip_spcor_constants(*args) == -1
        assert words in _ffi.error_buffer(), (words, _ffi.error_buffer())
    lib.vips_hip_error_clear()


@pytest.mark.parametrize("op", ["fastcor", "spcor"])
def test_null_arguments(op):
    """The null checks come before anything that needs a device."""
    fn = getattr(lib, "vips_hip_" + op)
    out = ctypes.c_void_p()
    lib.vips_hip_error_clear()
    assert fn(None, None, ctypes.byref(out)) == -1
    assert ("%s: null argument" % op) in _ffi.error_buffer()
    lib.vips_hip_error_clear()


def test_the_limit_is_what_the_header_says():
    assert lib.vips_hip_correlation_step(2) == 64
    header = open(_ffi.HEADER_PATH).read()
    assert "#define VIPS_HIP_CORRELATION_MAX_SIDE 64" in header
    assert lib.vips_hip_correlation_step(0) > 0 and lib.vips_hip_correlation_step(1) > 0
