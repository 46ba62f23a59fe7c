"""The libvips module's round_hip, sign_hip, clamp_hip, remainder_const_hip and recomb_hip (host/vips_hip_classes.c)
against the built-in operations through Ref.run: on the device whole and strip by strip (a small $VIPS_HIP_BUDGET, as
tests/test_module.py), bit for bit; and, where no GPU is present, what they hand to the original -- complex images,
more constants than the kernels keep, matrices above 32 x 32."""
import ctypes
import os

import numpy as np
import pytest

from tests import helpers
from tests.helpers import Ref
from tests.test_arith2_gpu import same_bits
from tests.test_arith_gpu import noise

# (on host fibers the library under test is not the one the module was linked against)
pytestmark = pytest.mark.skipif(not helpers.have_module() or bool(os.environ.get("VIPS_HIP_LIBRARY")),
                                reason="host/_build missing, or another build of the library is under test")

INTERP = helpers.INTERP
SEPIA = [[0.393, 0.769, 0.189], [0.349, 0.686, 0.168], [0.272, 0.534, 0.131]]


def matrix_file(tmp_path, m, name="m.v"):
    path = str(tmp_path / name)
    helpers.write_v(path, np.asarray(m, np.float64)[:, :, None], INTERP["multiband"])
    return path


@pytest.mark.gpu
@pytest.mark.parametrize("strips", [False, True], ids=["whole", "strips"])
def test_module_arith2_classes(tmp_path, strips):
    Ref.load_module()
    module = ctypes.CDLL(helpers.MODULE_LIB)
    height = 700 if strips else 50
    rgb = noise(400, height, np.uint8, 3, 801, with_extremes=True)
    grey = noise(400, height, np.uint16, 1, 803)
    signed = noise(400, height, np.int16, 3, 805, with_extremes=True)
    real = noise(400, height, np.float32, 3, 807, with_extremes=True)
    sepia, weights = matrix_file(tmp_path, SEPIA), matrix_file(tmp_path, [[0.2126, 0.7152, 0.0722]], "w.v")
    cases = [("round", real, "round=rint"), ("round", real, "round=ceil"), ("round", real, "round=floor"), ("round", rgb, "round=ceil"),
             ("sign", signed, ""), ("sign", real, ""), ("sign", rgb, ""),
             ("clamp", real, ""), ("clamp", rgb, "min=1.5,max=200.7"), ("clamp", signed, "min=-20.5,max=33.9"),
             ("remainder_const", rgb, "c=7"), ("remainder_const", signed, "c=3 0 -5"), ("remainder_const", grey, "c=3 0 5"),
             ("remainder_const", real, "c=2.7"),
             ("recomb", rgb, "m=" + sepia), ("recomb", real, "m=" + sepia), ("recomb", signed, "m=" + weights)]
    if strips:
        os.environ["VIPS_HIP_BUDGET"] = "300k"
    before = module.vips_hip_module_strips_done()
    try:
        for nick, src, args in cases:
            same_bits(Ref.run(nick + "_hip", src, args, interpretation=INTERP["srgb"]),
                      Ref.run(nick, src, args, interpretation=INTERP["srgb"]), "%s_hip %s" % (nick, args))
    finally:
        if strips:
            del os.environ["VIPS_HIP_BUDGET"]
    if strips:
        # (round of an integer image is the original's copy at every size)
        assert module.vips_hip_module_strips_done() - before >= 4 * (len(cases) - 1), "not strip-mined"


@pytest.mark.gpu
def test_module_errors_are_the_originals(tmp_path):
    Ref.load_module()
    src = noise(40, 30, np.uint8, 3, 811)
    with pytest.raises(RuntimeError, match="vector must have 1 or 3 elements"):
        Ref.run("remainder_const_hip", src, "c=1 2")
    with pytest.raises(RuntimeError, match="bands in must equal matrix width"):
        Ref.run("recomb_hip", src, "m=" + matrix_file(tmp_path, [[1.0, 2.0]]))


def test_module_hands_over_to_the_originals(tmp_path):
    """What never reaches the device (also on a box without a GPU): complex images, more constants than the kernels
    keep, a matrix above 32 x 32."""
    Ref.load_module()
    rng = np.random.default_rng(7)
    z = (rng.random((7, 9, 2)) + 1j * rng.random((7, 9, 2))).astype(np.complex64)
    for nick, args in (("round", "round=floor"), ("sign", ""), ("clamp", "min=0.2,max=0.6")):
        got, want = Ref.run(nick + "_hip", z, args), Ref.run(nick, z, args)
        assert got.dtype == want.dtype and np.array_equal(got, want), nick
    for nick, args in (("remainder_const", "c=3"), ("recomb", "m=" + matrix_file(tmp_path, [[1.0, 0.5], [0.0, 2.0]]))):
        with pytest.raises(RuntimeError, match="image must be non-complex"):
            Ref.run(nick + "_hip", z, args)
    wide = rng.integers(0, 255, (5, 6, 33)).astype(np.uint8)
    c = "c=" + " ".join(str(2 + k) for k in range(33))
    assert np.array_equal(Ref.run("remainder_const_hip", wide, c), Ref.run("remainder_const", wide, c))
    big = matrix_file(tmp_path, rng.normal(0, 1, (2, 33)), "big.v")
    got, want = Ref.run("recomb_hip", wide, "m=" + big), Ref.run("recomb", wide, "m=" + big)
    assert got.dtype == want.dtype and np.array_equal(got.view(np.uint32), want.view(np.uint32))
