"""GPU parity: vips_labelregions and vips_countlines on the device (libvips_amd/csrc/regions.hip, ops_regions.cpp).

Everything is equality -- np.array_equal on the mask with dtype, shape and interpretation, == on segments and on the
number of lines -- against the compiled reference, reached through its command line on .v files
(tests/regions_model.py).  countlines prints six decimals there, so beside that text the number is held to the double
the reference's own average is: its projection of its thresholded, convolved image, added in double, divided by the
number of sums and by 255.0.  Sizes go round the tile of label_tiles (vips_hip_labelregions_step).  Every labelregions
case asserts by the gate report that the six passes ran once each (the seam pass not where there is one tile)."""
import numpy as np
import pytest

import libvips_amd
from libvips_amd import Image, VipsHipError, _ffi
from tests import helpers
from tests import regions_model as model

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not helpers.have_ref(), reason="oracle/_ref not built")]

lib = _ffi.lib
TW, TH = lib.vips_hip_labelregions_step(0), lib.vips_hip_labelregions_step(1)
PASSES = ("label_tiles", "label_seams", "label_roots", "label_scan", "label_serials", "label_number")
FORMATS = [np.uint8, np.uint16, np.int32, np.float32, np.float64]
ALL_FORMATS = [np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32, np.float32, np.float64]
name_of = lambda d: np.dtype(d).name  # noqa: E731


@pytest.fixture(scope="module", autouse=True)
def _init():
    libvips_amd.init(0)


def label(src):
    """-> (mask (h, w), the mask image's header, segments) from the device, with the passes checked."""
    im = Image.new_from_array(src)
    lib.vips_hip_gate_reset()
    lib.vips_hip_gate_enable(1)
    try:
        out, opts = im.labelregions(with_options=True)
        report = {k: n for k, (n, _) in libvips_amd.gate_report().items()}
    finally:
        lib.vips_hip_gate_enable(0)
        lib.vips_hip_gate_reset()
    h, w = src.shape[:2]
    one_tile = w <= TW and h <= TH
    assert report == {k: 1 for k in PASSES if not (one_tile and k == "label_seams")}, report
    assert sorted(opts) == ["segments"]
    mask = out.numpy()
    assert (out.width, out.height, out.bands) == (w, h, 1)
    return mask[:, :, 0], (mask.dtype, out.interpretation), opts["segments"]


def check(tmp_path, src, what=None):
    want, interpretation, segments = model.ref_labelregions(tmp_path, src)
    got, (dtype, got_interpretation), got_segments = label(src)
    assert dtype == want.dtype == np.int32 and got.shape == want.shape, what
    assert got_interpretation == "multiband" and interpretation == model.MULTIBAND, what
    assert got_segments == segments, (what, got_segments, segments)
    assert np.array_equal(got, want), what
    return segments


# ------------------------------------------------------------------ labelregions

@pytest.mark.parametrize("w, h", [(1, 1), (1, TH + 1), (TW + 1, 1), (2 * TW + 1, 2 * TH + 1)])
def test_constant_is_one_region(tmp_path, w, h):
    assert check(tmp_path, model.constant(w, h, 9)) == 2


def test_checkerboard_is_all_regions(tmp_path):
    w, h = 2 * TW + 1, TH + 1
    assert check(tmp_path, model.checkerboard(w, h)) == w * h + 1


@pytest.mark.parametrize("period", [2, 3])
def test_diagonal_stripes_are_not_connected(tmp_path, period):
    """4- against 8-connectivity: a one-pel diagonal stripe is no region."""
    w, h = 2 * TW + 1, TH + 1
    segments = check(tmp_path, model.diagonal(w, h, period))
    if period == 2:
        assert segments == w * h + 1


def test_spiral(tmp_path):
    """Two regions, each crossing every seam many times: the longest chains label_seams and label_roots meet."""
    assert check(tmp_path, model.spiral(3 * TW + 1, 3 * TH + 1)) == 3


@pytest.mark.parametrize("name", ["arms in two tiles", "arms in one tile", "many", "comb"])
def test_u_shapes(tmp_path, name):
    """A region whose raster-first pel is far from where the tile pass first meets it."""
    w, h = 2 * TW + 1, 2 * TH + 1
    src = {"arms in two tiles": lambda: model.u_shape(w, h, 3, TW + 5, TH + 2),
           "arms in one tile": lambda: model.u_shape(w, h, 3, TW - 2, TH - 3),
           "many": lambda: model.many_us(w, h),
           "comb": lambda: model.comb(w, h)}[name]()
    check(tmp_path, src, name)


SIZES = [(w, h) for w in (TW - 1, TW, TW + 1, 2 * TW + 1) for h in (TH - 1, TH, TH + 1, 2 * TH + 1)]


@pytest.mark.parametrize("bands", [1, 3, 4])
@pytest.mark.parametrize("dtype", FORMATS, ids=name_of)
def test_noise(tmp_path, dtype, bands):
    """Two and four values a band at every size round the tile; pels of 1, 2, 3, 4, 6, 8, 12, 16, 24 and 32 bytes."""
    for i, (w, h) in enumerate(SIZES):
        values = 2 if i % 2 == 0 or bands > 1 else 4
        check(tmp_path, model.band_noise(w, h, bands, dtype, values, seed=11 + i), (w, h, values))
    check(tmp_path, model.band_noise(TW + 1, TH + 1, bands, dtype, 4, seed=5), "four values")


@pytest.mark.parametrize("dtype", FORMATS, ids=name_of)
def test_pels_that_differ_in_their_last_byte(tmp_path, dtype):
    for values in (2, 4):
        check(tmp_path, model.last_byte(model.noise(TW + 1, TH + 1, values, seed=3), dtype, 3), values)


def test_bytewise_equality(tmp_path):
    """+0.0 and -0.0 are two regions, NaNs of one payload one, NaNs of two payloads two: blocks that cross the seams."""
    w, h = 2 * TW + 2, 2 * TH + 2
    bits = np.empty((h, w), np.uint32)
    bits[:h // 2, :w // 2], bits[:h // 2, w // 2:] = 0x00000000, 0x80000000
    bits[h // 2:, :w // 2], bits[h // 2:, w // 2:] = 0x7fc00000, 0x7fc00001
    assert check(tmp_path, bits.view(np.float32)) == 5
    zeros = np.zeros((h, w), np.float32)
    zeros[:, w // 2:] = -0.0
    assert check(tmp_path, zeros) == 3
    nans = np.full((h, w), np.nan, np.float64)
    assert check(tmp_path, nans) == 2


def test_planes_are_rewritten_by_every_call(tmp_path):
    a = model.noise(2 * TW + 1, 2 * TH + 1, 2, seed=21)
    b = model.noise(TW + 3, TH + 5, 4, seed=22)
    first = label(a)
    second = label(a)
    assert first[2] == second[2] and np.array_equal(first[0], second[0])
    check(tmp_path, b, "another size")
    third = label(a)
    assert first[2] == third[2] and np.array_equal(first[0], third[0])
    check(tmp_path, a, "the first image again")


def test_without_options():
    src = model.checkerboard(5, 3)
    mask = Image.new_from_array(src).labelregions()
    assert np.array_equal(mask.numpy()[:, :, 0], np.arange(1, 16, dtype=np.int32).reshape(3, 5))


# ------------------------------------------------------------------ countlines

def check_lines(tmp_path, src, what=None):
    im = Image.new_from_array(src)
    a = src if src.ndim == 3 else src[:, :, None]
    h, w, b = a.shape
    for direction in model.DIRECTIONS:
        lib.vips_hip_gate_reset()
        lib.vips_hip_gate_enable(1)
        try:
            got = im.countlines(direction)
            report = {k: n for k, (n, _) in libvips_amd.gate_report().items()}
        finally:
            lib.vips_hip_gate_enable(0)
            lib.vips_hip_gate_reset()
        assert report == {"countlines": 1}, report
        assert "%f" % got == model.ref_countlines(tmp_path, src, direction), (what, direction, got)
        sums = model.ref_rises(tmp_path, src, direction)
        assert sums.size == (w if direction == "horizontal" else h) * b
        # vips_avg: the sums added in double, / the number of them; countlines.c:118: / 255.0
        want = float(sums.astype(np.float64).sum()) / float(sums.size) / 255.0
        assert got == want, (what, direction, got, want)


def test_countlines_example(tmp_path):
    src = np.array([[0, 255, 0, 255, 255], [0, 255, 0, 0, 255], [255, 0, 0, 255, 0]], np.uint8)
    check_lines(tmp_path, src)
    im = Image.new_from_array(src)
    assert im.countlines("horizontal") == 2 / 5 and im.countlines("vertical") == 5 / 3


@pytest.mark.parametrize("h", [1, 2, 63, 64, 65])
def test_countlines_noise(tmp_path, h):
    for w in (1, 2, 63, 64, 65):
        check_lines(tmp_path, helpers.lcg_image(w, h, 1, np.uint8, 31 + w), (w, h))
    # an extent x bands that is no power of two, on both axes
    check_lines(tmp_path, helpers.lcg_image(7, h, 3, np.uint8, 41), (7, h, 3))


@pytest.mark.parametrize("dtype", ALL_FORMATS, ids=name_of)
def test_countlines_formats(tmp_path, dtype):
    """Values on both sides of 128 and exactly 127 and 128, in every format, 1 .. 4 bands."""
    levels = np.array([0, 100, 127, 128, 129, 200], np.float64)
    if np.dtype(dtype).kind == "i":
        levels = np.concatenate([levels, [-128, -1]])
    if np.dtype(dtype).kind == "f":
        levels = np.concatenate([levels, [127.5, 127.99999, -300.0, 1e6]])
    if np.dtype(dtype).itemsize > 1:
        levels = np.concatenate([levels, [255, 256, 30000]])
    for bands in (1, 2, 3, 4):
        pick = helpers.lcg_image(37, 21, bands, np.uint8, 50 + bands) % len(levels)
        with np.errstate(over="ignore"):
            check_lines(tmp_path, levels[pick].astype(dtype), bands)


def test_countlines_second_turn(tmp_path):
    """More strips than a launch has in flight: rows of a little over 65 536 uchar elements (257 blocks, the last
    ragged, so seven strips in flight) and nine strips, the last ragged.  On the second turn a strip's first row looks
    at the row above it, which another block's first turn owned: noise, so a rise lost or counted twice there moves the
    count, in both directions."""
    threads, strip, most = (lib.vips_hip_countlines_step(i) for i in range(3))
    width = 256 * threads + 17
    blocks_x = -(-width // threads)
    in_flight = most // blocks_x
    height = (in_flight + 2) * strip - 5
    assert width % threads and in_flight >= 1 and -(-height // strip) > in_flight and height % strip
    check_lines(tmp_path, helpers.lcg_image(width, height, 1, np.uint8, 61), (width, height))


def test_countlines_constant(tmp_path):
    src = np.full((9, 70, 3), 200, np.uint8)
    check_lines(tmp_path, src)
    assert Image.new_from_array(src).countlines("horizontal") == 0.0


# ------------------------------------------------------------------ refusals

def test_refusals():
    comp = Image.new_from_array(np.zeros((4, 4, 1), np.complex64))
    with pytest.raises(VipsHipError, match="labelregions: complex images are outside the HIP path"):
        comp.labelregions()
    with pytest.raises(VipsHipError, match="countlines: complex images are outside the HIP path"):
        comp.countlines("horizontal")
    wide = Image.new_from_array(np.zeros((4, 4, 5), np.float64))
    with pytest.raises(VipsHipError, match="labelregions: pels of more than 32 bytes are outside the HIP path"):
        wide.labelregions()
    out, segments = _ffi.ctypes.c_void_p(), _ffi.ctypes.c_int()
    lib.vips_hip_error_clear()
    assert lib.vips_hip_labelregions(None, _ffi.ctypes.byref(out), _ffi.ctypes.byref(segments)) == -1
    assert "labelregions: null argument" in _ffi.error_buffer()
    lib.vips_hip_error_clear()
    with pytest.raises(ValueError, match="unknown direction"):
        Image.new_from_array(np.zeros((4, 4), np.uint8)).countlines("diagonal")
