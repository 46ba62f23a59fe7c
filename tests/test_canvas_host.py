"""CPU: the host side of the canvas operations (libvips_amd/csrc/ops_canvas.cpp) against the compiled reference -- no
GPU.

  - vips_hip_embed_need, the input rectangle a canvas rect draws on, against brute force over every pel of the rect,
    for all six extends on small geometries: the bounding box, exactly;
  - vips_hip_vector_to_ink, the ink of `background`, against what the reference paints;
  - vips_hip_embed_plan / vips_hip_gravity_position, the build() decisions (the identity copy, a background without an
    extend, the errors and their words, white in pels wider than a byte), against the reference;
  - (the header of every operation -- size, bands, format, interpretation -- needs the device to be asked for: it is
    checked against the reference in tests/test_canvas_gpu.py, which runs here too, on host fibers);
  - the C ABI of the feature is there with the signatures libvips_amd/_ffi.py declares."""
import ctypes

import numpy as np
import pytest

from libvips_amd import Image, _ffi
from tests import helpers
from tests.helpers import Ref

pytestmark = pytest.mark.skipif(not helpers.have_ref(), reason="oracle/_ref not built")

lib = _ffi.lib
EXTENDS = {"black": 0, "copy": 1, "repeat": 2, "mirror": 3, "white": 4, "background": 5}
DIRECTIONS = ["centre", "north", "east", "south", "west", "north-east", "south-east", "south-west", "north-west"]


def source_coordinate(extend, size, t):
    """Where coordinate t of the embedded axis reads an image of `size`: None for ink."""
    if 0 <= t < size:
        return t
    if extend == "copy":
        return min(max(t, 0), size - 1)
    if extend == "repeat":
        return t % size
    if extend == "mirror":
        m = t % (2 * size)
        return m if m < size else 2 * size - 1 - m
    return None


def brute_need(extend, iw, ih, x, y, left, top, width, height):
    xs = [source_coordinate(extend, iw, c - x) for c in range(left, left + width)]
    ys = [source_coordinate(extend, ih, r - y) for r in range(top, top + height)]
    xs, ys = [v for v in xs if v is not None], [v for v in ys if v is not None]
    if not xs or not ys:
        return None
    return (min(xs), min(ys), max(xs) - min(xs) + 1, max(ys) - min(ys) + 1)


@pytest.mark.parametrize("extend", sorted(EXTENDS))
def test_embed_need_is_brute_force(extend):
    need = (ctypes.c_int * 4)()
    checked = 0
    for iw, ih in ((1, 1), (1, 4), (3, 2), (5, 7)):
        for x, y in ((0, 0), (-2, 1), (3, -5), (-11, -9), (9, 14), (-1, -1)):
            for left in (0, 1, 4, 13):
                for width in (1, 2, 3, 5, 8, 11, 23):
                    for top, height in ((0, 1), (2, 3), (5, 9), (1, 16)):
                        lib.vips_hip_embed_need(EXTENDS[extend], iw, ih, x, y, left, top, width, height, need)
                        want = brute_need(extend, iw, ih, x, y, left, top, width, height)
                        if want is None:
                            assert need[2] == 0 or need[3] == 0, (iw, ih, x, y, left, top, width, height, tuple(need))
                        else:
                            assert tuple(need) == want, (iw, ih, x, y, left, top, width, height)
                        checked += 1
    assert checked == 4 * 6 * 4 * 7 * 4


def ink(background, bands, dtype):
    bg = np.atleast_1d(np.asarray(background, np.float64))
    out = np.zeros(bands, dtype)
    r = lib.vips_hip_vector_to_ink(bg.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), len(bg), bands,
                                   helpers.DTYPE_FORMATS[np.dtype(dtype)], out.ctypes.data)
    return out if r == 0 else None


@pytest.mark.parametrize("dtype", [np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32, np.float32, np.float64],
                         ids=lambda d: np.dtype(d).name)
def test_the_ink_is_the_reference(dtype):
    """The corner pel of embed(extend=background) is vips__vector_to_ink's pel: values inside, outside and between the
    values of every format, one value and one a band."""
    for bands in (1, 3):
        src = np.zeros((2, 2, bands), dtype)
        for background in (0, 7, 255.9, 256, -1.5, -129, 32767.5, 65535.2, 65536, 70000.7, 2.0 ** 31, 2.0 ** 32, 2.0 ** 33,
                           -2.0 ** 31 - 5, -2.0 ** 40, 16777217.0, 0.1, [1.25, -300, 1e10]):
            if isinstance(background, list) and bands == 1:
                continue
            args = "x=1,y=1,width=4,height=4,extend=background,background=" + " ".join(
                repr(float(v)) for v in np.atleast_1d(background))
            want = Ref.run("embed", src, args)[0, 0]
            got = ink(background, bands, dtype)
            assert got is not None and np.array_equal(got.view(np.uint8), want.view(np.uint8)), (background, bands, got, want)
    lib.vips_hip_error_clear()
    assert ink([1, 2], 3, dtype) is None and "linear: vector must have 1 or 3 elements" in _ffi.error_buffer()
    lib.vips_hip_error_clear()
    assert ink([1, 2, 3], 1, dtype) is not None  # a one-band image takes any vector (vips_check_vector)


def plan(nick, iw, ih, bands, fmt, interp, x, y, w, h, extend=None, background=None):
    args = Image.embed_args(extend, background)
    mode, ext = ctypes.c_int(-1), ctypes.c_int(-1)
    pel = np.zeros(32, np.uint8)
    lib.vips_hip_error_clear()
    r = lib.vips_hip_embed_plan(nick.encode(), ctypes.byref(args), iw, ih, bands, fmt, interp, x, y, w, h, ctypes.byref(mode),
                                ctypes.byref(ext), pel.ctypes.data)
    message = _ffi.error_buffer().strip()
    lib.vips_hip_error_clear()
    return r, mode.value, ext.value, pel, message


def test_embed_plan_decisions_and_error_texts():
    # the identity comes first, before the extend and the ink
    assert plan("embed", 8, 6, 3, 0, 22, 0, 0, 8, 6, "background", [1, 2])[:2] == (0, 0)
    # a background without an extend selects extend background; with one it does not
    assert plan("embed", 8, 6, 3, 0, 22, 1, 0, 9, 6, None, [5])[:3] == (0, 1, EXTENDS["background"])
    assert plan("embed", 8, 6, 3, 0, 22, 1, 0, 9, 6, "copy", [5])[:3] == (0, 1, EXTENDS["copy"])
    assert plan("embed", 8, 6, 3, 0, 22, 1, 0, 9, 6)[:3] == (0, 1, EXTENDS["black"])
    src = np.zeros((6, 8, 3), np.uint8)
    for extend in sorted(EXTENDS):
        for x, y, w, h in ((8, 0, 8, 6), (0, 6, 8, 6), (-8, 0, 8, 6), (0, -6, 8, 7), (100, 100, 5, 5), (7, 5, 8, 6)):
            r, mode, ext, _, message = plan("embed", 8, 6, 3, 0, 22, x, y, w, h, extend)
            try:
                Ref.run("embed", src, "x=%d,y=%d,width=%d,height=%d,extend=%s" % (x, y, w, h, extend))
                assert r == 0 and mode == 1, (extend, x, y, w, h, message)
            except RuntimeError as e:
                assert r == -1 and str(e).strip().endswith(message) and message == "embed: bad dimensions", (str(e), message)
    r, _, _, _, message = plan("gravity", 8, 6, 3, 0, 22, 40, 0, 9, 6)
    assert r == -1 and message == "gravity: bad dimensions"
    r, _, _, _, message = plan("embed", 8, 6, 3, 0, 22, 1, 0, 9, 6, "background", [1, 2])
    assert r == -1 and message == "linear: vector must have 1 or 3 elements"
    with pytest.raises(RuntimeError, match="linear: vector must have 1 or 3 elements"):
        Ref.run("embed", src, "x=1,y=0,width=9,height=6,extend=background,background=1 2")
    r, _, _, _, message = plan("embed", 8, 6, 2, 7, 0, 1, 0, 9, 6)
    assert r == -1 and message == "embed: image must be non-complex"


@pytest.mark.parametrize("dtype", [np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32, np.float32, np.float64],
                         ids=lambda d: np.dtype(d).name)
def test_white_is_what_the_reference_paints(dtype):
    fmt = helpers.DTYPE_FORMATS[np.dtype(dtype)]
    src = np.zeros((2, 2, 2), dtype)
    for interp in (0, 1, 22, 25, 26, 28):
        want = Ref.run("embed", src, "x=1,y=1,width=4,height=4,extend=white", interpretation=interp)[0, 0]
        r, mode, ext, pel, message = plan("embed", 2, 2, 2, fmt, interp, 1, 1, 4, 4, "white")
        assert r == 0 and ext == EXTENDS["white"], message
        assert np.array_equal(pel[:want.nbytes], want.view(np.uint8)), (interp, pel[:want.nbytes], want)


def test_gravity_positions_are_the_reference():
    """The marked pel of a one-pel image lands where vips_gravity puts it."""
    src = np.full((3, 5, 1), 9, np.uint8)
    src[0, 0, 0] = 200
    x, y = ctypes.c_int(), ctypes.c_int()
    for k, direction in enumerate(DIRECTIONS):
        for w, h in ((5, 3), (6, 4), (11, 8), (12, 3)):
            assert lib.vips_hip_gravity_position(k, 5, 3, w, h, ctypes.byref(x), ctypes.byref(y)) == 0
            want = Ref.run("gravity", src, "direction=%s,width=%d,height=%d" % (direction, w, h))[:, :, 0]
            assert want[y.value, x.value] == 200 and (want == 200).sum() == 1, (direction, w, h, x.value, y.value)
    lib.vips_hip_error_clear()
    assert lib.vips_hip_gravity_position(9, 5, 3, 7, 7, ctypes.byref(x), ctypes.byref(y)) == -1
    assert "gravity: enum 'VipsCompassDirection' has no member 9" in _ffi.error_buffer()
    lib.vips_hip_error_clear()


def test_the_abi_is_there():
    names = ["vips_hip_embed", "vips_hip_gravity", "vips_hip_flatten", "vips_hip_addalpha", "vips_hip_insert", "vips_hip_join",
             "vips_hip_embed_gen", "vips_hip_embed_need", "vips_hip_flatten_gen", "vips_hip_embed_defaults",
             "vips_hip_flatten_defaults", "vips_hip_insert_defaults", "vips_hip_embed_plan", "vips_hip_gravity_position",
             "vips_hip_vector_to_ink", "vips_hip_canvas_step"]
    header = open(_ffi.HEADER_PATH).read()
    for name in names:
        assert name in _ffi._SIGNATURES and name not in _ffi.MISSING, name
        assert getattr(lib, name).argtypes == _ffi._SIGNATURES[name][1]
        assert "VIPS_HIP_API" in header and name + "(" in header, name
    for method in ("embed", "gravity", "flatten", "addalpha", "insert", "join"):
        assert callable(getattr(Image, method))
    # the defaults, and the structs as the header lays them out
    e, f, i = _ffi.Embed(), _ffi.Flatten(), _ffi.Insert()
    e.extend, f.max_alpha_set, i.align = 3, 1, 2
    lib.vips_hip_embed_defaults(ctypes.byref(e))
    lib.vips_hip_flatten_defaults(ctypes.byref(f))
    lib.vips_hip_insert_defaults(ctypes.byref(i))
    assert (e.extend, e.extend_set, e.n_background) == (0, 0, 0)
    assert (f.n_background, f.max_alpha_set) == (0, 0) and (i.expand, i.shim, i.align, i.n_background) == (0, 0, 0, 0)
    assert ctypes.sizeof(_ffi.Embed) == 16 + 32 * 8 and ctypes.sizeof(_ffi.Flatten) == 8 + 32 * 8 + 16
    assert ctypes.sizeof(_ffi.Insert) == 8 + 32 * 8 + 8
    # the groups of the streaming kernel: whole pels and whole 16-byte groups
    assert lib.vips_hip_canvas_step(0, 0) == 256
    assert [lib.vips_hip_canvas_step(1, p) for p in (1, 2, 3, 4, 5, 6, 8, 12, 16, 24, 32)] == [16, 16, 48, 16, 0, 48, 16, 48, 16, 0, 0]
