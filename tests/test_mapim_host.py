"""CPU: the host side of vips_mapim (libvips_amd/csrc/ops_mapim.cpp): the defaults, the need of a generate rect from the
bounds of its index (resample/mapim.c:145-224 and :351-365, restated here in numpy), the Python argument handling.
No device is touched."""
import ctypes
import math

import numpy as np
import pytest

from libvips_amd import Image, VipsHipError, _ffi

lib = _ffi.lib
MAX_COORD = 10000000  # VIPS_MAX_COORD's default
INTERPOLATORS = {"nearest": (1, 0), "bilinear": (2, 0), "bicubic": (4, 1)}  # window_size, window_offset (interpolate.c:150-167)
EXTENDS = ("black", "copy", "repeat", "mirror", "white", "background")
INDEX_DTYPES = [np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32, np.float32, np.complex64, np.float64, np.complex128]


def test_defaults():
    args = _ffi.Mapim()
    ctypes.memset(ctypes.byref(args), 0xFF, ctypes.sizeof(args))
    lib.vips_hip_mapim_defaults(ctypes.byref(args))
    assert (args.interpolate, args.extend, args.premultiplied, args.n_background) == (1, 5, 0, 1)
    assert list(args.background) == [0.0] * _ffi.Mapim.MAX_BACKGROUND
    assert ctypes.sizeof(args) == 4 * 4 + 8 * 64
    lib.vips_hip_mapim_defaults(None)  # (returns)


def model_need(bounds, interpolate, extend, width, height):
    """mapim.c:207-223 and :351-365 on the extremes of the index's components, then the embedded rect as pels of the
    image (what the fetch reads for it, as vips_hip_affine_need reports it)."""
    window_size, window_offset = INTERPOLATORS[interpolate]
    clip = lambda v: max(-1.0, min(float(MAX_COORD), v))  # noqa: E731
    min_x, min_y = clip(float(np.floor(bounds[0]))), clip(float(np.floor(bounds[1])))
    max_x, max_y = clip(float(np.ceil(bounds[2]))), clip(float(np.ceil(bounds[3])))
    b_left, b_top = int(min_x), int(min_y)
    b_width, b_height = int((max_x - min_x) + 1), int((max_y - min_y) + 1)
    n_left, n_top = b_left + 1, b_top + 1
    n_width, n_height = b_width + window_size - 1, b_height + window_size - 1
    # vips_rect_intersectrect with the embedded image
    e_width, e_height = width + window_size - 1 + 2, height + window_size - 1 + 2
    x0, y0 = max(n_left, 0), max(n_top, 0)
    x1, y1 = min(n_left + n_width, e_width), min(n_top + n_height, e_height)
    if x1 <= x0 or y1 <= y0:
        return [0, 0, 0, 0]
    off = window_offset + 1

    def axis(e0, e1, size):
        if (e0 < off or e1 >= off + size) and extend in ("repeat", "mirror"):
            return 0, size - 1
        return min(max(e0 - off, 0), size - 1), min(max(e1 - off, 0), size - 1)

    px0, px1 = axis(x0, x1 - 1, width)
    py0, py1 = axis(y0, y1 - 1, height)
    return [px0, py0, px1 - px0 + 1, py1 - py0 + 1]


def device_need(bounds, interpolate, extend, width, height):
    args = Image.mapim_args(interpolate=interpolate, extend=extend)
    b = (ctypes.c_double * 4)(*bounds)
    need = (ctypes.c_int * 4)(-9, -9, -9, -9)
    _ffi.check(lib.vips_hip_mapim_bounds_need(b, ctypes.byref(args), width, height, need))
    return list(need)


def edge_values(dtype, size):
    """The values of this index format round the clip edges -1 and VIPS_MAX_COORD, round 0 and round the image."""
    dt = np.dtype(dtype)
    if dt.kind in "ui":
        info = np.iinfo(dt)
        cand = [info.min, info.min + 1, -3, -2, -1, 0, 1, 2, size - 2, size - 1, size, size + 1, size + 5, MAX_COORD - 1, MAX_COORD,
                MAX_COORD + 1, info.max - 1, info.max]
        return sorted({float(v) for v in cand if info.min <= v <= info.max})
    part = np.float32 if dt in (np.dtype(np.float32), np.dtype(np.complex64)) else np.float64
    cand = [-np.inf, -1e30, -3.5, -1.0000001, -1.0, -0.9999999, -0.5, -1e-30, 0.0, 0.25, 1.0, 1.75, size - 1.5, size - 1.0, size - 0.25,
            size + 0.0, size + 0.5, size + 1.0, size + 7.25, MAX_COORD - 1.5, MAX_COORD - 1.0, MAX_COORD + 0.0, MAX_COORD + 1.0, 1e30, np.inf]
    return sorted({float(part(v)) for v in cand})


@pytest.mark.parametrize("dtype", INDEX_DTYPES, ids=lambda d: np.dtype(d).name)
def test_need_of_bounds(dtype):
    """Every pair min <= max of the format's edge values on one axis against a fixed other axis, under every
    interpolator and extend mode, for a 53 x 37 image."""
    width, height = 53, 37
    xs, ys = edge_values(dtype, width), edge_values(dtype, height)
    checked = 0
    for interpolate in INTERPOLATORS:
        for extend in EXTENDS:
            for i, lo in enumerate(xs):
                for hi in xs[i:]:
                    b = [lo, 3.0, hi, 9.0]
                    assert device_need(b, interpolate, extend, width, height) == model_need(b, interpolate, extend, width, height), \
                        (b, interpolate, extend)
                    checked += 1
            for i, lo in enumerate(ys):
                for hi in ys[i:]:
                    b = [10.0, lo, 20.0, hi]
                    assert device_need(b, interpolate, extend, width, height) == model_need(b, interpolate, extend, width, height), \
                        (b, interpolate, extend)
                    checked += 1
    assert checked > 500


def test_need_of_bounds_known_answers():
    # a rect that reads pels 10 .. 20 x 3 .. 9 exactly: the stencil's margin on every side
    assert device_need([10, 3, 20, 9], "nearest", "background", 53, 37) == [10, 3, 11, 7]
    assert device_need([10, 3, 20, 9], "bilinear", "background", 53, 37) == [10, 3, 12, 8]
    assert device_need([10, 3, 20, 9], "bicubic", "background", 53, 37) == [9, 2, 14, 10]
    # everything right of the embedded image, and a component without a number: all ink
    assert device_need([60, 3, 70, 9], "bicubic", "background", 53, 37) == [0, 0, 0, 0]
    assert device_need([math.inf, 3, -math.inf, 9], "bilinear", "copy", 53, 37) == [0, 0, 0, 0]
    # left of -1 the clip makes -1 of it: the embed's first column, which the fetch reads as the image's
    assert device_need([-50, 3, -40, 9], "bilinear", "background", 53, 37) == [0, 3, 1, 8]
    # a border under repeat and mirror: the whole axis
    assert device_need([-1, 3, 5, 9], "bilinear", "repeat", 53, 37) == [0, 3, 53, 8]
    assert device_need([10, 30, 20, 37], "bilinear", "mirror", 53, 37) == [10, 0, 12, 37]


def test_need_of_bounds_refuses():
    args = Image.mapim_args()
    b = (ctypes.c_double * 4)(0, 0, 1, 1)
    need = (ctypes.c_int * 4)(5, 5, 5, 5)
    for call in (lambda: lib.vips_hip_mapim_bounds_need(None, ctypes.byref(args), 5, 5, need),
                 lambda: lib.vips_hip_mapim_bounds_need(b, None, 5, 5, need),
                 lambda: lib.vips_hip_mapim_bounds_need(b, ctypes.byref(args), 0, 5, need),
                 lambda: lib.vips_hip_mapim_bounds_need(b, ctypes.byref(args), 5, 5, None)):
        lib.vips_hip_error_clear()
        assert call() == -1 and "mapim" in _ffi.error_buffer()
    args.interpolate = 7
    lib.vips_hip_error_clear()
    assert lib.vips_hip_mapim_bounds_need(b, ctypes.byref(args), 5, 5, need) == -1
    assert "interpolator 7 is outside the HIP path" in _ffi.error_buffer()
    assert list(need) == [0, 0, 0, 0]
    lib.vips_hip_error_clear()


def test_step_reports_the_units():
    assert lib.vips_hip_mapim_step(0) % lib.vips_hip_mapim_step(2) == 0
    assert lib.vips_hip_mapim_step(1) % lib.vips_hip_mapim_step(3) == 0
    assert lib.vips_hip_mapim_step(2) * lib.vips_hip_mapim_step(3) == 64  # a wave
    assert lib.vips_hip_mapim_step(5) % 64 == 0 and lib.vips_hip_mapim_step(6) == 16
    assert lib.vips_hip_mapim_step(99) == -1


def test_python_arguments():
    args = Image.mapim_args()
    assert (args.interpolate, args.extend, args.premultiplied, args.n_background, args.background[0]) == (1, 5, 0, 1, 0.0)
    args = Image.mapim_args(interpolate="bicubic", extend="mirror", background=[1, 2.5, 3], premultiplied=True)
    assert (args.interpolate, args.extend, args.premultiplied, args.n_background) == (2, 3, 1, 3)
    assert list(args.background[:4]) == [1.0, 2.5, 3.0, 0.0]
    assert Image.mapim_args(interpolate="NEAREST", background=7).background[0] == 7.0
    with pytest.raises(VipsHipError, match="mapim: interpolator lbb is outside the HIP path"):
        Image.mapim_args(interpolate="lbb")
    with pytest.raises(ValueError, match="unknown extend"):
        Image.mapim_args(extend="sideways")
    with pytest.raises(VipsHipError, match="background of more than 64 elements"):
        Image.mapim_args(background=[0] * 65)
    # the methods exist with pyvips' argument names
    import inspect

    assert list(inspect.signature(Image.mapim).parameters) == ["self", "index", "interpolate", "extend", "background", "premultiplied"]
    assert list(inspect.signature(Image.xyz).parameters) == ["width", "height"]
