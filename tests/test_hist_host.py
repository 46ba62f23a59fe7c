"""CPU: the host side of the histogram operations (libvips_amd/csrc/ops_histogram.cpp) against the compiled reference
-- no GPU.

  - vips_hip_hist_cum_host and vips_hip_hist_norm_host, the arithmetic under vips_hip_hist_cum / vips_hip_hist_norm /
    vips_hip_hist_equal, are the reference's hist_cum -> hist_norm -> cast chain on hand-made histograms: both loops
    of vips_linear (equal and different maxima a band), counts above 2^24 (the float conversion's loss), histograms
    narrower than 256, the ushort results of histograms of more than 256 entries, up to the 65536 vips_check_hist allows;
  - the C ABI of the feature is there with the signatures libvips_amd/_ffi.py declares, and the tiles the GPU tests
    size their images by are what include/vips_hip.h says."""
import ctypes

import numpy as np
import pytest

from libvips_amd import Image, _ffi
from tests import helpers
from tests.helpers import Ref

pytestmark = pytest.mark.skipif(not helpers.have_ref(), reason="oracle/_ref not built")

lib = _ffi.lib
PU = ctypes.POINTER(ctypes.c_uint)
HISTOGRAM = 10
NORM_DTYPES = {0: np.uint8, 2: np.uint16, 4: np.uint32}


def cum_host(h):
    h = np.ascontiguousarray(h, np.uint32)
    out = np.zeros_like(h)
    lib.vips_hip_hist_cum_host(h.ctypes.data_as(PU), h.shape[1], h.shape[2], out.ctypes.data_as(PU))
    return out


def norm_host(h):
    h = np.ascontiguousarray(h, np.uint32)
    raw = np.zeros(h.size, np.uint32)
    fmt = lib.vips_hip_hist_norm_host(h.ctypes.data_as(PU), h.shape[1], h.shape[2], raw.ctypes.data)
    return np.ascontiguousarray(raw.view(NORM_DTYPES[fmt])[:h.size].reshape(h.shape))


def histograms():
    out = []
    for b in (1, 3, 4):
        out.append(("noise %d" % b, Ref.run("hist_find", helpers.lcg_image(97, 41, b, np.uint8, 21 + b))))
        one = np.zeros((1, 256, b), np.uint32)
        one[0, 77, :] = 5000
        out.append(("one bin %d" % b, one))
        big = (helpers.lcg_image(256, 1, b, np.uint32, 31 + b) >> 9) + np.uint32(1 << 22)
        out.append(("large counts %d" % b, big))
        flat = np.full((1, 256, b), (1 << 24) + 3, np.uint32)
        flat[0, 0::2, :] = (1 << 23) + 1
        out.append(("large equal counts %d" % b, flat))
        out.append(("narrow %d" % b, np.ascontiguousarray(big[:, :10, :])))
        out.append(("one entry %d" % b, np.ascontiguousarray(big[:, :1, :])))
    out.append(("ushort out", helpers.lcg_image(300, 1, 2, np.uint32, 41) >> 12))
    out.append(("ushort out, the widest histogram", helpers.lcg_image(65536, 1, 1, np.uint32, 43) >> 18))
    return out


@pytest.mark.parametrize("case", histograms() if helpers.have_ref() else [], ids=lambda c: c[0])
def test_cum_norm_cast_is_the_reference(case):
    what, h = case
    want_cum = Ref.run("hist_cum", h, interpretation=HISTOGRAM)
    got_cum = cum_host(h)
    assert got_cum.dtype == want_cum.dtype and np.array_equal(got_cum, want_cum), what
    for src in (h, want_cum):
        want = Ref.run("hist_norm", src, interpretation=HISTOGRAM)
        got = norm_host(src)
        assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype)
        assert np.array_equal(got, want), (what, np.argwhere(got != want)[:4])
    # hist_equal's chain ends in a cast to the image's format: of a uchar table, to uchar
    if h.shape[1] <= 256:
        chain = Ref.run("cast", Ref.run("hist_norm", want_cum, interpretation=HISTOGRAM), "format=uchar")
        assert np.array_equal(norm_host(got_cum), chain), what


def test_the_abi_is_there():
    names = ["vips_hip_maplut", "vips_hip_hist_cum", "vips_hip_hist_norm", "vips_hip_hist_cum_host", "vips_hip_hist_norm_host",
             "vips_hip_hist_equal", "vips_hip_hist_local_gen", "vips_hip_hist_local_step", "vips_hip_hist_local",
             "vips_hip_stdif_gen", "vips_hip_stdif_step", "vips_hip_stdif"]
    header = open(_ffi.HEADER_PATH).read()
    for name in names:
        assert name in _ffi._SIGNATURES and name not in _ffi.MISSING, name
        assert getattr(lib, name).argtypes == _ffi._SIGNATURES[name][1]
        assert "VIPS_HIP_API" in header and name + "(" in header, name
    for method in ("hist_cum", "hist_norm", "hist_equal", "maplut", "hist_local", "stdif"):
        assert callable(getattr(Image, method))


def test_the_tiles():
    run, rows, side, lanes, count_area, count_elems, count_rows = [lib.vips_hip_hist_local_step(i) for i in range(7)]
    assert lib.vips_hip_hist_local_step(7) == 0
    assert run > 0 and rows > 0 and lanes >= 4 and count_elems > 0 and count_rows > 0
    assert side >= 64 and 1 <= count_area < 65535
    # the bins of a block and a 64 x 64 tile of 4-band pels fit a CU's LDS
    assert lanes * rows * 512 + (rows + 63) * ((lanes // 4 * run + 63) * 4 + 19) <= 160 * 1024
    assert lib.vips_hip_stdif_step(0) > 0 and lib.vips_hip_stdif_step(1) > 0
    assert lib.vips_hip_stdif_step(2) == 66051 and 255 * 255 * 66051 < 1 << 32 <= 255 * 255 * 66052
