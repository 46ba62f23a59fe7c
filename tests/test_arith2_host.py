"""CPU: the host side of round, sign, clamp, minpair, maxpair, remainder, remainder_const, recomb, sum and bandrank
(libvips_amd/csrc/ops_arith.cpp, ops_recomb.cpp, ops_nary.cpp) against the compiled reference -- the format tables of the
new enumerators over every format and every pair of formats, put to the reference by running the operation on 1 x 1
images; the planning of remainder_const's constants; recomb's header and refusals; the header of an array of images and
bandrank's index rule; the Python argument handling."""
import ctypes
import inspect
import math
import os
import subprocess

import numpy as np
import pytest

from libvips_amd import Image, _ffi
from libvips_amd.image import _enum
from tests import helpers
from tests.helpers import Ref

pytestmark = pytest.mark.skipif(not helpers.have_ref(), reason="oracle/_ref not built")

lib = _ffi.lib
INTERP = helpers.INTERP
VIPS = os.path.join(helpers.ROOT, "oracle", "_ref", "bin", "vips")
# VipsHipArith: the new enumerators follow the ones tests/test_arith_host.py pins
OPS = {"round": 7, "sign": 8, "clamp": 9, "minpair": 10, "maxpair": 11, "remainder": 12, "remainder_const": 13}
ARGS = {"round": "round=ceil", "sign": "", "clamp": "min=1,max=3", "remainder_const": "c=2"}
REAL = [np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32, np.float32, np.float64]


def test_the_enumerators_are_at_the_end():
    assert [lib.vips_hip_arith_format(op, 0) for op in range(7)] == [6, 0, 0, 2, 3, 2, 6]
    assert sorted(OPS.values()) == list(range(7, 14))
    assert lib.vips_hip_arith_format(14, 0) == -1
    for op in OPS.values():
        for fmt in (7, 9, -1, 10):
            assert lib.vips_hip_arith_format(op, fmt) == -1


@pytest.mark.parametrize("nick", sorted(ARGS))
def test_unary_format_tables(nick):
    for dtype in REAL:
        want = Ref.run(nick, np.array([[[2]]], dtype), ARGS[nick])
        assert helpers.FORMAT_DTYPES[lib.vips_hip_arith_format(OPS[nick], helpers.DTYPE_FORMATS[np.dtype(dtype)])] == want.dtype.type, (nick, dtype)


def plan(op, fa, fb):
    out = [ctypes.c_int() for _ in range(6)]
    lib.vips_hip_error_clear()
    if lib.vips_hip_binary_plan(OPS[op], 1, 1, 1, fa, INTERP["b-w"], 1, 1, 1, fb, INTERP["b-w"], *[ctypes.byref(v) for v in out]) != 0:
        message = _ffi.error_buffer().strip()
        lib.vips_hip_error_clear()
        raise RuntimeError(message)
    return tuple(v.value for v in out)


@pytest.mark.parametrize("op", ["minpair", "maxpair", "remainder"])
def test_binary_plan_formats(tmp_path, op):
    """Every pair of real formats: the output's format is the reference's, and the common format is the one whose
    arithmetic gives the reference's pixel (200 against 7; 200 is -56 as a char, and 200 again only where the common
    format of char and uchar is wide enough for both)."""
    paths = {}
    for t in REAL:
        for v in (200, 7):
            paths[t, v] = str(tmp_path / ("%s_%d.v" % (np.dtype(t).name, v)))
            helpers.write_v(paths[t, v], np.array([[[v]]]).astype(t), INTERP["b-w"])
    out = str(tmp_path / "out.v")
    for ta in REAL:
        for tb in REAL:
            r = subprocess.run([VIPS, op, paths[ta, 200], paths[tb, 7], out], env=helpers.ref_cli_env(), stdout=subprocess.PIPE,
                               stderr=subprocess.PIPE, text=True)
            assert r.returncode == 0, r.stderr
            pixels, interp = helpers.read_v(out)
            common, out_format, bands, pinterp, w, h = plan(op, helpers.DTYPE_FORMATS[np.dtype(ta)], helpers.DTYPE_FORMATS[np.dtype(tb)])
            assert (out_format, bands, pinterp, w, h) == (helpers.DTYPE_FORMATS[pixels.dtype], 1, interp, 1, 1), (op, ta, tb)
            assert out_format == common == lib.vips_hip_arith_format(OPS[op], common)
            ct = np.dtype(helpers.FORMAT_DTYPES[common])
            lo, hi = (np.iinfo(ct).min, np.iinfo(ct).max) if ct.kind in "ui" else (-np.inf, np.inf)
            x, y = (np.clip(np.array([[[v]]]).astype(t).astype(np.float64), lo, hi) for v, t in ((200, ta), (7, tb)))  # vips_cast clips
            # (% truncates for the integer formats, the float formats floor)
            want = {"minpair": np.minimum(x, y), "maxpair": np.maximum(x, y),
                    "remainder": np.fmod(x, y) if ct.kind in "ui" else x - y * np.floor(x / y)}[op]
            assert np.array_equal(pixels.astype(np.float64), want), (op, ta, tb, pixels, want)


def test_binary_plan_refuses_what_is_not_binary():
    for op in ("round", "sign", "clamp", "remainder_const"):
        with pytest.raises(RuntimeError, match="not a binary operation"):
            plan(op, 0, 0)
    with pytest.raises(RuntimeError, match="minpair: image must be non-complex"):
        plan("minpair", 7, 0)


def test_remainder_const_plan():
    """remainder_const reads c_int (remainder.c:277, :290): the constants truncated toward zero, one a band."""
    for c, bands in (([2.7], 3), ([2.7, -4.2, 0.9], 3), ([3, 0, 5], 1), ([-0.5], 1)):
        src = np.full((1, 1, bands), 7, np.int16)
        want = Ref.run("remainder_const", src, "c=" + " ".join(repr(float(v)) for v in c))
        out_bands = ctypes.c_int()
        ci = (ctypes.c_int * 32)()
        assert lib.vips_hip_const_plan(b"remainder_const", (ctypes.c_double * len(c))(*c), len(c), bands, 3, ctypes.byref(out_bands),
                                       None, ci, None) == 0
        assert out_bands.value == want.shape[2]
        # (C's % truncates, as math.fmod does)
        assert want.ravel().tolist() == [int(math.fmod(7, ci[k])) if ci[k] else -1 for k in range(out_bands.value)]
        assert list(ci[:out_bands.value]) == [int(c[min(k, len(c) - 1)]) for k in range(out_bands.value)]


def recomb_plan(bands, fmt, mw, mh, m_bands=1, m_fmt=8):
    out_bands, out_format = ctypes.c_int(), ctypes.c_int()
    lib.vips_hip_error_clear()
    if lib.vips_hip_recomb_plan(bands, fmt, mw, mh, m_bands, m_fmt, ctypes.byref(out_bands), ctypes.byref(out_format)) != 0:
        message = _ffi.error_buffer().strip()
        lib.vips_hip_error_clear()
        raise RuntimeError(message)
    return out_bands.value, out_format.value


def test_recomb_plan(tmp_path):
    """The output's bands and format for every format against the reference, its refusals in its words and order."""
    m = np.array([[0.5, 0.25, 0.125], [1.0, 2.0, 3.0]])
    helpers.write_v(str(tmp_path / "m.v"), m[:, :, None], 0)
    for dtype in REAL:
        helpers.write_v(str(tmp_path / "in.v"), np.full((1, 1, 3), 2, dtype), INTERP["srgb"])
        r = subprocess.run([VIPS, "recomb", str(tmp_path / "in.v"), str(tmp_path / "out.v"), str(tmp_path / "m.v")],
                           env=helpers.ref_cli_env(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert r.returncode == 0, r.stderr
        want, _ = helpers.read_v(str(tmp_path / "out.v"))
        assert recomb_plan(3, helpers.DTYPE_FORMATS[np.dtype(dtype)], 3, 2) == (want.shape[2], helpers.DTYPE_FORMATS[want.dtype])
        assert want.ravel().tolist() == [1.75, 12.0]
    # recomb.c:174-185, in that order; then this library's own limit
    for args, words in (((3, 7, 2, 2, 2, 9), "image must be non-complex"), ((3, 0, 2, 2, 2, 9), "image must be non-complex"),
                        ((3, 0, 2, 2, 2, 8), "image must one band"), ((3, 0, 2, 2, 1, 8), "bands in must equal matrix width"),
                        ((33, 0, 33, 2, 1, 8), "a matrix of 33 x 2 is outside the HIP path (at most 32 x 32)"),
                        ((3, 0, 3, 33, 1, 0), "a matrix of 3 x 33 is outside the HIP path (at most 32 x 32)")):
        with pytest.raises(RuntimeError) as info:
            recomb_plan(*args)
        assert str(info.value) == "recomb: " + words
    assert recomb_plan(32, 0, 32, 32) == (32, 6)


def nary_plan(rank, headers, index=-1):
    """headers: [(width, height, bands, format, interpretation)] -> (format, out_format, bands, interpretation, width, height, index)."""
    n = len(headers)
    columns = [(ctypes.c_int * n)(*[h[k] for h in headers]) for k in range(5)]
    out = [ctypes.c_int() for _ in range(7)]
    lib.vips_hip_error_clear()
    if lib.vips_hip_nary_plan(rank, n, *columns, index, *[ctypes.byref(v) for v in out]) != 0:
        message = _ffi.error_buffer().strip()
        lib.vips_hip_error_clear()
        raise RuntimeError(message)
    return tuple(v.value for v in out)


def ref_array(tmp_path, op, arrays, index=None):
    paths = []
    for i, (array, interp) in enumerate(arrays):
        paths.append(str(tmp_path / ("n%d.v" % i)))
        helpers.write_v(paths[-1], array, interp)
    out = str(tmp_path / "out.v")
    r = subprocess.run([VIPS, op, " ".join(paths), out] + (["--index", str(index)] if index is not None else []),
                       env=helpers.ref_cli_env(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if r.returncode != 0:
        raise RuntimeError(r.stderr.strip())
    return helpers.read_v(out)


@pytest.mark.parametrize("op", ["sum", "bandrank"])
def test_nary_plan_formats(tmp_path, op):
    """Every pair of real formats, and a third image of the first: the result's format is the reference's."""
    for ta in REAL:
        for tb in REAL:
            arrays = [(np.full((1, 1, 1), 3, t), INTERP["b-w"]) for t in (ta, tb, ta)]
            want, interp = ref_array(tmp_path, op, arrays)
            headers = [(1, 1, 1, helpers.DTYPE_FORMATS[np.dtype(t)], INTERP["b-w"]) for t in (ta, tb, ta)]
            common, out_format, bands, pinterp, w, h, index = nary_plan(op == "bandrank", headers)
            assert (out_format, bands, pinterp, w, h) == (helpers.DTYPE_FORMATS[want.dtype], 1, interp, 1, 1), (op, ta, tb)
            assert want.ravel().tolist() == [9 if op == "sum" else 3]


def test_nary_plan_bands_sizes_and_bandrank_index(tmp_path):
    def im(w, h, bands, interp):
        return np.ones((h, w, bands), np.uint8), INTERP[interp]

    def header(a):
        return a[0].shape[1], a[0].shape[0], a[0].shape[2], 0, a[1]

    cases = [[im(7, 5, 3, "srgb"), im(4, 9, 3, "srgb"), im(2, 2, 3, "srgb")], [im(7, 5, 1, "b-w"), im(4, 9, 3, "srgb"), im(4, 9, 1, "multiband")],
             [im(3, 3, 3, "multiband"), im(3, 3, 3, "srgb")], [im(3, 3, 1, "b-w"), im(3, 3, 4, "srgb"), im(3, 3, 4, "scrgb")],
             [im(3, 3, 3, "srgb"), im(3, 3, 4, "srgb")], [im(3, 3, 1, "b-w")]]
    for arrays in cases:
        for op in ("sum", "bandrank"):
            try:
                want, interp = ref_array(tmp_path, op, arrays)
            except RuntimeError as e:
                with pytest.raises(RuntimeError) as info:
                    nary_plan(op == "bandrank", [header(a) for a in arrays])
                assert str(info.value).split(": ", 1)[-1] in str(e) and str(info.value).startswith(op + ":")
                continue
            got = nary_plan(op == "bandrank", [header(a) for a in arrays])
            assert got[2:6] == (want.shape[2], interp, want.shape[1], want.shape[0]), (op, [a[0].shape for a in arrays], got)
    # bandrank.c:225-230: -1 is n / 2, an index of n or more is refused; one image is a copy whatever the index
    five = [(3, 3, 1, 0, 1)] * 5
    assert [nary_plan(1, five, i)[6] for i in (-1, 0, 1, 4)] == [2, 0, 1, 4]
    assert nary_plan(1, five[:4], -1)[6] == 2 and nary_plan(1, five[:2], -1)[6] == 1
    for index in (5, 6, -2):
        with pytest.raises(RuntimeError, match="bandrank: index out of range"):
            nary_plan(1, five, index)
    nary_plan(1, five[:1], 7)
    with pytest.raises(RuntimeError, match="sum: arrays of more than 16 images are outside the HIP path"):
        nary_plan(0, [(3, 3, 1, 0, 1)] * 17)
    with pytest.raises(RuntimeError, match="bandrank: arrays of more than 16 images are outside the HIP path"):
        nary_plan(1, [(3, 3, 1, 0, 1)] * 17)


def test_python_arguments():
    m = Image.recomb_matrix([[1, 2, 3], [4, 5, 6]])
    assert m.dtype == np.float64 and m.shape == (2, 3) and m.flags["C_CONTIGUOUS"]
    assert Image.recomb_matrix(np.arange(6, dtype=np.uint8).reshape(3, 2)[:, ::-1]).tolist() == [[1, 0], [3, 2], [5, 4]]
    assert Image.recomb_matrix([0.2, 0.7, 0.1]).shape == (1, 3) and Image.recomb_matrix(np.ones((2, 3, 1))).shape == (2, 3)
    for bad in ([], np.ones((2, 3, 2))):
        with pytest.raises(ValueError):
            Image.recomb_matrix(bad)
    assert list(inspect.signature(Image.recomb).parameters) == ["self", "m"]
    assert list(inspect.signature(Image.sum).parameters) == ["images"]
    rank = inspect.signature(Image.bandrank).parameters
    assert list(rank) == ["self", "other", "index"] and rank["index"].default == -1
    for bad in ([], [1, 2], None):
        with pytest.raises(TypeError):
            Image.sum(bad)
    assert [_enum(Image.ROUND, k, "round") for k in ("rint", "CEIL", "floor", 1)] == [0, 1, 2, 1]
    with pytest.raises(ValueError, match="unknown round 'nearest'"):
        _enum(Image.ROUND, "nearest", "round")
    assert list(inspect.signature(Image.round).parameters) == ["self", "round"]
    clamp = inspect.signature(Image.clamp).parameters
    assert list(clamp) == ["self", "min", "max"] and (clamp["min"].default, clamp["max"].default) == (0.0, 1.0)
    for name in ("rint", "ceil", "floor", "sign"):
        assert list(inspect.signature(getattr(Image, name)).parameters) == ["self"]
    for name in ("minpair", "maxpair", "remainder"):
        assert list(inspect.signature(getattr(Image, name)).parameters) == ["self", "other"]
    assert Image.__mod__ is Image.remainder
