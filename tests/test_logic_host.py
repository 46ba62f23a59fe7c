"""CPU: the host side of the mask operations (libvips_amd/csrc/ops_logic.cpp) against the compiled reference -- the
format tables for all ten formats, the format, band, size and interpretation decisions of relational / boolean over all
format pairs and of ifthenelse and bandjoin over mixed images (headers straight from the reference's command line and
its build()), the constants' classification (c_int, c_double, is_int), the refusals in the reference's words.  No device
is touched."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from libvips_amd import _ffi
from tests import helpers
from tests.helpers import Ref

pytestmark = pytest.mark.skipif(not helpers.have_ref(), reason="oracle/_ref not built")

lib = _ffi.lib
INTERP = helpers.INTERP
VIPS = os.path.join(helpers.ROOT, "oracle", "_ref", "bin", "vips")
REAL = [np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32, np.float32, np.float64]


def call(fn, *args):
    lib.vips_hip_error_clear()
    if fn(*args) != 0:
        message = _ffi.error_buffer().strip()
        lib.vips_hip_error_clear()
        raise RuntimeError(message)


def header_args(images):
    args = []
    for array, interp in images:
        h, w, bands = array.shape
        args += [w, h, bands, helpers.DTYPE_FORMATS[array.dtype], interp]
    return args


def ref_header(tmp_path, op, images, *args):
    """(format, bands, interpretation, width, height) of the reference's command line on these images."""
    paths = []
    for i, (array, interp) in enumerate(images):
        paths.append(str(tmp_path / ("in%d.v" % i)))
        helpers.write_v(paths[-1], array, interp)
    out = str(tmp_path / "out.v")
    ins = [" ".join(paths)] if op == "bandjoin" else paths
    r = subprocess.run([VIPS, op] + ins + [out] + list(args), env=helpers.ref_cli_env(), stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True)
    if r.returncode != 0:
        raise RuntimeError(r.stderr.strip().splitlines()[-1])
    array, interp = helpers.read_v(out)
    return helpers.DTYPE_FORMATS[array.dtype], array.shape[2], interp, array.shape[1], array.shape[0]


def logic_plan(boolean, a, b):
    out = [ctypes.c_int() for _ in range(6)]
    call(lib.vips_hip_logic_plan, boolean, *header_args([a, b]), *[ctypes.byref(v) for v in out])
    return tuple(v.value for v in out)  # format, out_format, bands, interpretation, width, height


def im(w, h, bands, interp, dtype=np.uint8):
    return np.ones((h, w, bands), dtype), INTERP[interp]


def test_format_tables():
    """All ten formats: the built operation's format is the table's (complex formats: the table's entry, though the
    device path refuses those images)."""
    for fmt, dtype in enumerate([np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32, np.float32, np.complex64, np.float64,
                                 np.complex128]):
        src = np.ones((1, 2, 2), dtype)
        assert lib.vips_hip_logic_format(0, fmt) == helpers.DTYPE_FORMATS[Ref.run("relational_const", src, "relational=more,c=1").dtype]
        if np.dtype(dtype).kind != "c":
            assert lib.vips_hip_logic_format(1, fmt) == helpers.DTYPE_FORMATS[Ref.run("boolean_const", src, "boolean=and,c=1").dtype]
            assert lib.vips_hip_logic_format(1, fmt) == helpers.DTYPE_FORMATS[Ref.run("bandbool", src, "boolean=and").dtype]
        else:
            assert lib.vips_hip_logic_format(1, fmt) == 5
    assert lib.vips_hip_logic_format(0, 10) == -1 and lib.vips_hip_logic_format(1, -1) == -1


@pytest.mark.parametrize("op", [("relational", "less", 0), ("boolean", "eor", 1)], ids=lambda o: o[0])
def test_logic_plan_formats(tmp_path, op):
    nick, arg, boolean = op
    for ta in REAL:
        for tb in REAL:
            a, b = im(2, 1, 1, "b-w", ta), im(2, 1, 1, "b-w", tb)
            fmt, bands, interp, w, h = ref_header(tmp_path, nick, [a, b], arg)
            common, out_format, pbands, pinterp, pw, ph = logic_plan(boolean, a, b)
            assert (out_format, pbands, pinterp, pw, ph) == (fmt, bands, interp, w, h), (nick, ta, tb)
            assert out_format == lib.vips_hip_logic_format(boolean, common)


def test_logic_plan_bands_sizes_and_interpretations(tmp_path):
    cases = [(im(7, 5, 3, "srgb"), im(4, 9, 3, "srgb")), (im(7, 5, 1, "b-w"), im(4, 9, 3, "srgb")),
             (im(7, 5, 3, "srgb"), im(4, 9, 1, "b-w")), (im(3, 3, 3, "multiband"), im(3, 3, 3, "srgb")),
             (im(3, 3, 3, "srgb"), im(3, 3, 3, "multiband")), (im(3, 3, 1, "multiband"), im(3, 3, 4, "srgb", np.uint16)),
             (im(3, 3, 1, "b-w"), im(2, 2, 1, "multiband")), (im(3, 3, 3, "srgb"), im(3, 3, 4, "srgb")),
             (im(3, 3, 4, "srgb"), im(3, 3, 2, "multiband")), (im(3, 3, 2, "multiband"), im(3, 3, 5, "multiband"))]
    for a, b in cases:
        for nick, arg, boolean in (("relational", "more", 0), ("boolean", "and", 1)):
            try:
                want = ref_header(tmp_path, nick, [a, b], arg)
            except RuntimeError as e:
                with pytest.raises(RuntimeError) as info:
                    logic_plan(boolean, a, b)
                assert str(info.value) == str(e), (str(e), str(info.value))
                continue
            assert logic_plan(boolean, a, b)[1:] == want, (nick, a[0].shape, b[0].shape)


def test_ifthenelse_plan(tmp_path):
    shapes = [(im(9, 7, 1, "b-w"), im(9, 7, 3, "srgb"), im(9, 7, 3, "srgb", np.int16)),
              (im(9, 7, 3, "srgb"), im(9, 7, 1, "b-w", np.uint16), im(9, 7, 1, "b-w", np.float32)),
              (im(9, 7, 3, "multiband"), im(9, 7, 1, "b-w"), im(9, 7, 3, "srgb")),
              (im(9, 7, 3, "lab", np.float32), im(9, 7, 1, "b-w"), im(9, 7, 1, "multiband")),
              (im(4, 9, 1, "b-w"), im(9, 7, 3, "srgb"), im(5, 5, 3, "multiband", np.float64)),
              (im(9, 7, 1, "b-w"), im(9, 7, 3, "srgb"), im(9, 7, 4, "srgb")),
              (im(9, 7, 2, "multiband"), im(9, 7, 3, "srgb"), im(9, 7, 3, "srgb"))]
    for images in shapes:
        out = [ctypes.c_int() for _ in range(5)]
        try:
            want = ref_header(tmp_path, "ifthenelse", list(images))
        except RuntimeError as e:
            with pytest.raises(RuntimeError) as info:
                call(lib.vips_hip_ifthenelse_plan, *header_args(images), *[ctypes.byref(v) for v in out])
            assert str(info.value) == str(e), (str(e), str(info.value))
            continue
        call(lib.vips_hip_ifthenelse_plan, *header_args(images), *[ctypes.byref(v) for v in out])
        assert tuple(v.value for v in out) == want, [i[0].shape for i in images]


def test_bandjoin_plan(tmp_path):
    sets = [[im(9, 7, 3, "srgb"), im(9, 7, 1, "b-w")], [im(9, 7, 1, "b-w"), im(4, 9, 3, "srgb", np.int16), im(9, 7, 2, "multiband", np.uint16)],
            [im(3, 3, 1, "b-w", t) for t in REAL], [im(2, 2, 2, "multiband", np.uint32), im(2, 2, 2, "multiband", np.int8)]]
    for images in sets:
        n = len(images)
        arrays = [(ctypes.c_int * n)(*[a.shape[k] for a, _ in images]) for k in (1, 0, 2)]
        formats = (ctypes.c_int * n)(*[helpers.DTYPE_FORMATS[a.dtype] for a, _ in images])
        out = [ctypes.c_int() for _ in range(5)]
        call(lib.vips_hip_bandjoin_plan, n, *arrays, formats, images[0][1], *[ctypes.byref(v) for v in out])
        assert tuple(v.value for v in out) == ref_header(tmp_path, "bandjoin", images)
    with pytest.raises(RuntimeError, match="no input images"):
        call(lib.vips_hip_bandjoin_plan, 0, arrays[0], arrays[1], arrays[2], formats, 0, *[ctypes.byref(v) for v in out])


def const_plan(nick, c, bands, dtype):
    c = np.atleast_1d(np.asarray(c, np.float64))
    out_bands, is_int = ctypes.c_int(), ctypes.c_int()
    ci, cd = (ctypes.c_int * 32)(), (ctypes.c_double * 32)()
    call(lib.vips_hip_const_plan, nick.encode(), c.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), len(c), bands,
         helpers.DTYPE_FORMATS[np.dtype(dtype)], ctypes.byref(out_bands), ctypes.byref(is_int), ci, cd)
    return out_bands.value, bool(is_int.value), list(ci)[:out_bands.value], list(cd)[:out_bands.value]


def test_const_plan():
    """Bands, the vector-length errors in the reference's words, c_int / c_double / is_int; which comparison the
    reference took shows in its pixels: 3 > 2.5 but not 3 > (int) 2.5 + 1."""
    for bands in (1, 2, 3):
        src = np.full((1, 2, bands), 3, np.uint8)
        for c in ([2], [2.5], [1, 2], [1, 2, 3], [1.5, 2, 3], [1, 2, 3, 4], [-1e10], [3e9]):
            for nick, arg in (("relational_const", "relational=more"), ("boolean_const", "boolean=and")):
                try:
                    want = Ref.run(nick, src, "%s,c=%s" % (arg, " ".join(repr(float(x)) for x in c)))
                except RuntimeError as e:
                    with pytest.raises(RuntimeError) as info:
                        const_plan(nick, c, bands, np.uint8)
                    assert nick + ": " + str(info.value) == str(e).strip().splitlines()[-1], (str(e), str(info.value))
                    continue
                out_bands, is_int, ci, cd = const_plan(nick, c, bands, np.uint8)
                assert out_bands == want.shape[2], (bands, c)
                assert cd == [float(c[min(i, len(c) - 1)]) for i in range(out_bands)]
                assert is_int == all(float(x).is_integer() and abs(x) < 2 ** 31 for x in c), (c, is_int)
                if is_int:
                    assert ci == [int(x) for x in cd]
    assert const_plan("relational_const", [2.5], 1, np.uint8)[2] == [2]
    # is_int against what the reference itself does: on a uint image `> c` is 0 everywhere where it compared with the
    # int constant made unsigned (a negative c) and 255 everywhere where it compared doubles
    u = np.array([0, 7, 4294967295], np.uint32).reshape(1, 3, 1)
    for c in (-1, -1.5, -2, -2.25, -1e10, -2147483648, -2147483649):
        took_int = Ref.run("relational_const", u, "relational=more,c=%r" % float(c)).ravel().tolist() != [255, 255, 255]
        assert const_plan("relational_const", [c], 1, np.uint32)[1] == took_int, c
    # c_int of constants outside int: boolean_const uses it whatever is_int says; `| c` shows it in the pixels
    for c in (1e10, -1e10, 3e9, 2147483648.0, -2147483649.0):
        want = Ref.run("boolean_const", np.zeros((1, 1, 1), np.int32), "boolean=or,c=%r" % c).ravel().tolist()
        assert const_plan("boolean_const", [c], 1, np.int32)[2] == want, (c, want)
    with pytest.raises(RuntimeError, match="image must be non-complex"):
        const_plan("boolean_const", [1], 1, np.complex64)


def test_refusals():
    """What never reaches a device: null arguments, a shift across bands, a band out of range, too many images."""
    out = ctypes.c_void_p()
    for fn, args in ((lib.vips_hip_relational, (None, None, ctypes.byref(out), 0)), (lib.vips_hip_ifthenelse, (None, None, None, None, 0)),
                     (lib.vips_hip_bandjoin, (None, 2, ctypes.byref(out))), (lib.vips_hip_extract_band, (None, ctypes.byref(out), 0, 1)),
                     (lib.vips_hip_bandmean, (None, None))):
        with pytest.raises(RuntimeError, match="null argument"):
            call(fn, *args)
    for op, nick in ((3, "lshift"), (4, "rshift")):
        with pytest.raises(RuntimeError, match="operator %s not supported across image bands" % nick):
            call(lib.vips_hip_bandbool, None, ctypes.byref(out), op)
    with pytest.raises(RuntimeError, match="bad operation"):
        call(lib.vips_hip_bandbool, None, ctypes.byref(out), 7)
