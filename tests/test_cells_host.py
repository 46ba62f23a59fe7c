"""CPU: the host side of the sheet operations (libvips_amd/csrc/ops_cells.cpp) -- no GPU.

  - vips_hip_arrayjoin_plan, the geometry of vips_arrayjoin_build on plain ints (the output's size, every image's rect
    and the offset of the image in it), against the numpy model of tests/cells_model.py, which a few cases pin to the
    compiled reference through its command line: the three aligns, images smaller and larger than the spacing (offsets
    of either sign), shims, incomplete last rows;
  - vips_hip_replicate_need and vips_hip_grid_need against brute force over every pel of the rect;
  - the reference's words for the errors of grid and subsample, which tests/test_cells_gpu.py (here: on host fibers)
    then finds in the library's messages."""
import ctypes

import numpy as np
import pytest

from libvips_amd import _ffi
from tests import cells_model as model
from tests import helpers
from tests.helpers import Ref

lib = _ffi.lib
needs_ref = pytest.mark.skipif(not helpers.have_ref(), reason="oracle/_ref not built")
ALIGN_CODES = {"low": 0, "centre": 1, "high": 2}


def lib_plan(sizes, across=None, shim=0, halign="low", valign="low", hspacing=None, vspacing=None):
    n = len(sizes)
    args = _ffi.Arrayjoin()
    lib.vips_hip_arrayjoin_defaults(ctypes.byref(args))
    args.across, args.shim = across or 0, shim
    args.halign, args.valign = ALIGN_CODES[halign], ALIGN_CODES[valign]
    args.hspacing, args.vspacing = hspacing or 0, vspacing or 0
    widths, heights = (ctypes.c_int * n)(*[w for w, _ in sizes]), (ctypes.c_int * n)(*[h for _, h in sizes])
    width, height, across_out = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    rects, offsets = (ctypes.c_int * (4 * n))(), (ctypes.c_int * (2 * n))()
    _ffi.check(lib.vips_hip_arrayjoin_plan(ctypes.byref(args), n, widths, heights, ctypes.byref(width), ctypes.byref(height),
                                           ctypes.byref(across_out), rects, offsets))
    return (width.value, height.value, across_out.value, [tuple(rects[4 * i:4 * i + 4]) for i in range(n)],
            [tuple(offsets[2 * i:2 * i + 2]) for i in range(n)])


SIZES = [(7, 5), (4, 9), (12, 3), (1, 1), (6, 6), (9, 2), (5, 5)]


@pytest.mark.parametrize("halign", model.ALIGNS)
@pytest.mark.parametrize("valign", model.ALIGNS)
def test_the_plan_is_the_model(halign, valign):
    """Spacings from the largest image, and given: smaller than some images (negative offsets, odd and even slack),
    larger than all of them."""
    checked = 0
    for n in (1, 2, 3, 5, 7):
        for across in (None, 1, 2, 3, 9):
            for shim in (0, 1, 4):
                for hspacing, vspacing in ((None, None), (5, 4), (6, 3), (20, 11), (None, 2)):
                    kw = dict(across=across, shim=shim, halign=halign, valign=valign, hspacing=hspacing, vspacing=vspacing)
                    assert lib_plan(SIZES[:n], **kw) == model.plan(SIZES[:n], **kw), (n, kw)
                    checked += 1
    assert checked == 5 * 5 * 3 * 5


def test_the_plan_in_numbers():
    """Three images of 4 x 3, 2 x 5 and 7 x 2 across 2 with a shim of 1, centred: the boxes are 7 x 5; the rects of the
    first column and row take the shim; the last image's rect reaches the right edge; the slack is halved toward zero."""
    width, height, across, rects, offsets = lib_plan([(4, 3), (2, 5), (7, 2)], across=2, shim=1, halign="centre", valign="centre")
    assert (width, height, across) == (15, 11, 2)
    assert rects == [(0, 0, 8, 6), (8, 0, 7, 6), (0, 6, 15, 5)]
    assert offsets == [(1, 1), (2, 0), (0, 1)]
    # boxes of 3 x 2: every image is cropped; high puts the image's far edge on the box's
    _, _, _, _, offsets = lib_plan([(4, 3), (2, 5), (7, 2)], across=2, halign="high", valign="centre", hspacing=3, vspacing=2)
    assert offsets == [(-1, 0), (1, -1), (-4, 0)]


@needs_ref
def test_the_model_is_the_reference(tmp_path):
    """The model's pixels (and so its plan) against the reference's command line: each align with images smaller and
    larger than the spacing, a shim, an incomplete last row."""
    arrays = [np.ascontiguousarray(helpers.lcg_image(w, h, 3, np.uint8, 40 + i)) for i, (w, h) in enumerate(SIZES[:5])]
    images = [(a, helpers.INTERP["srgb"]) for a in arrays]
    for align in model.ALIGNS:
        for kw in (dict(across=3, shim=2), dict(across=2, hspacing=5, vspacing=4), dict(across=4, shim=1, hspacing=6, vspacing=3)):
            kw.update(halign=align, valign=align, background=[7, 8, 9])
            want, _ = model.ref_arrayjoin(tmp_path, images, model.cli_options(**kw))
            ink = np.array(kw["background"], np.uint8)
            got = model.arrayjoin(arrays, ink, **{k: v for k, v in kw.items() if k != "background"})
            assert got.shape == want.shape and np.array_equal(got, want), (align, kw)


def test_plan_errors():
    lib.vips_hip_error_clear()
    for kw, words in ((dict(across=1000001), "out of range"), (dict(shim=-1), "out of range")):
        with pytest.raises(_ffi.VipsHipError, match="arrayjoin: .*" + words):
            lib_plan(SIZES[:2], **kw)
    with pytest.raises(_ffi.VipsHipError, match="arrayjoin: output size overflows an int"):
        lib_plan([(1000000, 1)] * 3000, across=3000)
    with pytest.raises(_ffi.VipsHipError, match="arrayjoin: no input images"):
        lib_plan([])


def need_of(fn, *args):
    need = (ctypes.c_int * 4)()
    fn(*(args + (need,)))
    return tuple(need)


def box(xs, ys):
    return (min(xs), min(ys), max(xs) - min(xs) + 1, max(ys) - min(ys) + 1)


def test_replicate_need_is_brute_force():
    checked = 0
    for w, h in ((1, 1), (3, 2), (5, 7)):
        for x0, y0 in ((0, 0), (2 % w, 1 % h), (w, h)):
            for left in (0, 1, 4, 13):
                for width in (1, 2, 3, 5, 8):
                    for top, height in ((0, 1), (2, 3), (5, 9)):
                        xs = [(c + x0) % w for c in range(left, left + width)]
                        ys = [(r + y0) % h for r in range(top, top + height)]
                        got = need_of(lib.vips_hip_replicate_need, w, h, x0, y0, left, top, width, height)
                        assert got == box(xs, ys), (w, h, x0, y0, left, top, width, height)
                        checked += 1
    assert checked == 3 * 3 * 4 * 5 * 3


def test_grid_need_is_brute_force():
    """The bounding box of the strip's pels that a rect of the grid shows: one tile's columns and rows for a rect inside
    a tile, every column and the rows from the first tile's to the last tile's once it spans tiles across."""
    w, checked = 4, 0
    for tile_height, across, down in ((3, 1, 4), (2, 3, 2), (1, 4, 3), (5, 2, 2)):
        h = tile_height * across * down
        for left in range(0, w * across, 3):
            for width in (1, 2, w, w + 1, w * across - left):
                if left + width > w * across:
                    continue
                for top in range(0, tile_height * down, 2):
                    for height in (1, 2, tile_height, tile_height * down - top):
                        if top + height > tile_height * down:
                            continue
                        xs, ys = [], []
                        for Y in range(top, top + height):
                            for X in range(left, left + width):
                                tx, ty = X // w, Y // tile_height
                                xs.append(X - tx * w)
                                ys.append((ty * across + tx) * tile_height + Y - ty * tile_height)
                        got = need_of(lib.vips_hip_grid_need, w, h, tile_height, across, left, top, width, height)
                        want = box(xs, ys)
                        # (a rect that spans tiles across is given every column)
                        if left // w != (left + width - 1) // w:
                            want = (0, want[1], w, want[3])
                        assert got == want, (tile_height, across, down, left, top, width, height)
                        checked += 1
    assert checked > 300


@needs_ref
def test_the_references_words():
    """What vips_grid and vips_subsample say (the library's messages are checked against these words where the device
    runs); vips_subsample names its image argument "input"."""
    src = np.ascontiguousarray(helpers.lcg_image(8, 12, 3, np.uint8, 50))
    with pytest.raises(RuntimeError, match="grid: bad grid geometry"):
        Ref.run("grid", src, "tile_height=5,across=1,down=2")
    with pytest.raises(RuntimeError, match="grid: bad grid geometry"):
        Ref.run("grid", src, "tile_height=4,across=2,down=2")
    assert Ref.run("grid", src, "tile_height=4,across=3,down=1").shape == (4, 24, 3)
    with pytest.raises(RuntimeError, match="subsample: image has shrunk to nothing"):
        model.ref_input("subsample", src, "xfac=9,yfac=1")
    with pytest.raises(RuntimeError, match="subsample: image has shrunk to nothing"):
        model.ref_input("subsample", src, "xfac=1,yfac=13")
    got, _ = model.ref_input("subsample", src, "xfac=3,yfac=5")
    assert np.array_equal(got, src[::5][:2, ::3][:, :2])
    with pytest.raises(RuntimeError, match="zoom: zoom factors too large"):
        model.ref_input("zoom", np.ascontiguousarray(helpers.lcg_image(120, 2, 1, np.uint8, 51)), "xfac=10000000,yfac=1")
