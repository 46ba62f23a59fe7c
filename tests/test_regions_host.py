"""CPU: the plain-Python model of vips_labelregions / vips_countlines (tests/regions_model.py) against the compiled
reference on every pattern the device tests use, so that a failure of tests/test_regions_gpu.py points at a kernel and
not at the model or a pattern; what the new entry points say without a device."""
import ctypes

import numpy as np
import pytest

from libvips_amd import _ffi
from tests import helpers
from tests import regions_model as model

lib = _ffi.lib
needs_ref = pytest.mark.skipif(not helpers.have_ref(), reason="oracle/_ref not built")

TW, TH = lib.vips_hip_labelregions_step(0), lib.vips_hip_labelregions_step(1)


def test_steps():
    assert TW >= 8 and TH >= 2
    assert lib.vips_hip_labelregions_step(2) == 32
    assert lib.vips_hip_labelregions_step(3) == 0 and lib.vips_hip_labelregions_step(-1) == 0


def patterns():
    w, h = 2 * TW + 1, TH + 1
    yield "constant", model.constant(w, h)
    yield "one pel", model.constant(1, 1)
    yield "checkerboard", model.checkerboard(w, h)
    yield "diagonal 2", model.diagonal(w, h, 2)
    yield "diagonal 3", model.diagonal(w, h, 3)
    yield "spiral", model.spiral(3 * TW + 1, 3 * TH + 1)
    yield "u across tiles", model.u_shape(2 * TW + 1, 2 * TH + 1, 3, TW + 5, TH + 2)
    yield "many us", model.many_us(2 * TW + 1, 2 * TH + 1)
    yield "comb", model.comb(2 * TW + 1, 2 * TH + 1)
    yield "noise 2", model.noise(TW + 1, TH + 1, 2)
    yield "noise 4", model.noise(TW + 1, TH + 1, 4)
    yield "noise 2 x 3 double", model.band_noise(TW - 1, TH + 1, 3, np.float64, 2)
    yield "last byte", model.last_byte(model.noise(TW + 1, TH - 1, 4), np.uint16, 3)


@needs_ref
@pytest.mark.parametrize("name, src", list(patterns()), ids=[n for n, _ in patterns()])
def test_model_labelregions_is_the_reference(tmp_path, name, src):
    want, interpretation, segments = model.ref_labelregions(tmp_path, src)
    got, got_segments = model.labelregions(src)
    assert interpretation == model.MULTIBAND and want.dtype == np.int32
    assert got_segments == segments
    assert np.array_equal(got, want)


def test_model_on_the_issue_example():
    src = np.array([[1, 0, 1, 1], [0, 1, 0, 1], [1, 1, 0, 1]], np.uint8)
    mask, segments = model.labelregions(src)
    assert mask.tolist() == [[1, 2, 3, 3], [4, 5, 6, 3], [5, 5, 6, 3]] and segments == 7


def test_patterns_are_what_they_claim():
    w, h = 2 * TW + 1, TH + 1
    assert model.labelregions(model.checkerboard(w, h))[1] == w * h + 1
    assert model.labelregions(model.diagonal(w, h, 2))[1] == w * h + 1
    assert model.labelregions(model.constant(w, h))[1] == 2
    # the spiral and what it leaves are one region each
    assert model.labelregions(model.spiral(3 * TW + 1, 3 * TH + 1))[1] == 3
    # a U's first pel is the top of its right arm
    mask, _ = model.labelregions(model.u_shape(2 * TW + 1, 2 * TH + 1, 3, TW + 5, TH + 2))
    assert mask[TH + 2, 3] == mask[0, TW + 5] == 2


@needs_ref
def test_model_bytewise_equality_is_the_reference(tmp_path):
    src = bytewise_blocks()
    want, _, segments = model.ref_labelregions(tmp_path, src)
    got, got_segments = model.labelregions(src)
    assert got_segments == segments == 5 and np.array_equal(got, want)


def bytewise_blocks():
    """+0.0 | -0.0 over NaN (payload 0) | NaN (payload 1), blocks of 3 x 2: four regions."""
    bits = np.empty((4, 6), np.uint32)
    bits[:2, :3], bits[:2, 3:], bits[2:, :3], bits[2:, 3:] = 0x00000000, 0x80000000, 0x7fc00000, 0x7fc00001
    return bits.view(np.float32)


COUNT_EXAMPLE = np.array([[0, 255, 0, 255, 255], [0, 255, 0, 0, 255], [255, 0, 0, 255, 0]], np.uint8)


def test_model_countlines_on_the_issue_example():
    assert model.countlines(COUNT_EXAMPLE, "horizontal") == 2 / 5
    assert model.countlines(COUNT_EXAMPLE, "vertical") == 5 / 3 == (255.0 * 5) / 3.0 / 255.0


def count_inputs():
    yield "example", COUNT_EXAMPLE
    yield "noise 7 x 5 x 3", helpers.lcg_image(7, 5, 3, np.uint8, 3)
    yield "noise 65 x 2", helpers.lcg_image(65, 2, 1, np.uint8, 4)
    yield "one column", helpers.lcg_image(1, 63, 1, np.uint8, 5)
    yield "char", helpers.lcg_image(9, 7, 2, np.int8, 6)
    yield "short", (helpers.lcg_image(9, 7, 1, np.int16, 7) >> 7)
    yield "float", helpers.lcg_image(9, 7, 3, np.float32, 8)
    yield "edges of 128", np.array([[127, 128, 127.5, 128.5, 127, 129]], np.float64).T.copy()
    yield "constant", np.full((5, 6), 200, np.uint8)


@needs_ref
@pytest.mark.parametrize("direction", model.DIRECTIONS)
@pytest.mark.parametrize("name, src", list(count_inputs()), ids=[n for n, _ in count_inputs()])
def test_model_countlines_is_the_reference(tmp_path, name, src, direction):
    # what the reference prints, and the integers its average is made of
    assert "%f" % model.countlines(src, direction) == model.ref_countlines(tmp_path, src, direction)
    sums = model.ref_rises(tmp_path, src, direction)
    assert int(sums.sum()) == 255 * model.rises(src, direction)


def test_null_arguments_are_errors():
    out, segments, nolines = ctypes.c_void_p(), ctypes.c_int(), ctypes.c_double()
    lib.vips_hip_error_clear()
    assert lib.vips_hip_labelregions(None, ctypes.byref(out), ctypes.byref(segments)) == -1
    assert "labelregions: null argument" in _ffi.error_buffer()
    lib.vips_hip_error_clear()
    assert lib.vips_hip_countlines(None, 0, ctypes.byref(nolines)) == -1
    assert "countlines: null argument" in _ffi.error_buffer()
    lib.vips_hip_error_clear()
