"""GPU parity: vips_rank / vips_median and vips_morph (libvips_amd/csrc/rank.hip, morph.hip, ops_morphology.cpp).

Both operations are exact -- an order statistic, bitwise logic on bytes -- so every comparison is np.array_equal
against the compiled reference, shapes and dtypes included.  Every case asserts which kernel family ran, by the gate
report.  Sizes are taken round the kernels' tiles (vips_hip_rank_step): T_w elements x T_h rows.

The cases are a sparse cross, not the full product window x index x size x bands x format (a few hundred thousand
reference calls that would say nothing more): what a kernel does depends on its family (which window and index pick
it), on the element size, and on where the image's edges fall in the tile, so
  - every window x every index x every band count runs on uchar at three sizes: the window itself, the window + 1,
    and one tile + 1 (test_rank_windows);
  - every size round the tile (widths x heights, the full 4 x 4) x every band count runs for one window per kernel
    family (test_rank_sizes_round_the_tile);
  - every other format runs the 3 x 3, 5 x 5 and 11 x 11 windows with every index at one tile + 1, bands 1 and 3
    (test_rank_formats).
A numpy model of the operation, anchored on the reference, then sweeps odd sizes, windows and band counts the lists
above do not hold (test_rank_sweep_against_the_model).  vips_morph is crossed the same way: every mask x both
operations x both kinds of input x every band count at one size, one mask over every size round the tile.
Float inputs are positive noise: no NaN, no -0 (include/vips_hip.h says what the device defines for those).
Runs on the CPU too, on host fibers (tests/test_emul_rank_morph.py)."""
import ctypes
import os

import numpy as np
import pytest

import libvips_amd
from libvips_amd import Image, VipsHipError, _ffi
from tests import helpers
from tests.helpers import Ref

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not helpers.have_ref(), reason="oracle/_ref not built")]

lib = _ffi.lib
# (on host fibers the library under test is not the one the module was linked against)
needs_module = pytest.mark.skipif(not helpers.have_module() or bool(os.environ.get("VIPS_HIP_LIBRARY")),
                                  reason="host/_build missing, or another build of the library is under test")

WINDOWS = [(3, 3), (5, 5), (2, 2), (4, 3), (1, 7), (7, 1), (3, 4), (9, 10), (7, 13), (11, 11), (31, 31)]
BANDS = [1, 3, 4]


@pytest.fixture(scope="module", autouse=True)
def _init():
    libvips_amd.init(0)


class gated(object):
    """with gated() as g: ...; g.report: {gate name: (launches, ms)} of what ran inside."""

    def __enter__(self):
        lib.vips_hip_gate_reset()
        lib.vips_hip_gate_enable(1)
        self.report = None
        return self

    def __exit__(self, *exc):
        try:
            if exc[0] is None:
                self.report = libvips_amd.gate_report()
        finally:
            lib.vips_hip_gate_enable(0)
            lib.vips_hip_gate_reset()
        return False


def tiles():
    """((rank T_w, T_h), (morph T_w, T_h)); T_w in elements."""
    t = tuple(lib.vips_hip_rank_step(i) for i in range(4))
    assert all(v > 0 for v in t), t
    return t[:2], t[2:]


def round_the_tile(tile, bands):
    """Widths (pels) one under / at / over a tile's elements and two tiles + 5; heights the same for its rows."""
    tw, th = tile
    at = -(-tw // bands)
    return (at - 1, at, at + 1, 2 * at + 5), (th - 1, th, th + 1, 2 * th + 5)


def indexes(n):
    return sorted(set(i for i in (0, 1, n // 2, n - 2, n - 1) if 0 <= i < n))


def rank_family(w, h, index):
    n = w * h
    if index == 0 or index == n - 1:
        return "rank_minmax"
    return "rank_median3" if (w, h, index) == (3, 3, 4) else "rank_select"


_noise = {}


def noise(w, h, bands, dtype=np.uint8, seed=11):
    """A w x h corner of one big noise image per (bands, dtype, seed): made once, never changed."""
    key = (bands, np.dtype(dtype), seed)
    if key not in _noise or _noise[key].shape[0] < h or _noise[key].shape[1] < w:
        have = _noise.get(key)
        side_w = max(w, have.shape[1] if have is not None else 0, 700)
        side_h = max(h, have.shape[0] if have is not None else 0, 80)
        _noise[key] = helpers.lcg_image(side_w, side_h, bands, dtype, seed)
    return np.ascontiguousarray(_noise[key][:h, :w])


def same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d of %d differ, first at %s: got %r want %r" % (
            what, len(bad), got.size, bad[0], got[tuple(bad[0])], want[tuple(bad[0])]))


def run_rank(src, w, h, index):
    """Image.rank with the gate check: one launch of the expected family and of no other."""
    with gated() as g:
        got = Image.new_from_array(src).rank(w, h, index).numpy()
    ran = {k: n for k, (n, _) in g.report.items() if k.startswith("rank_")}
    assert ran == {rank_family(w, h, index): 1}, (w, h, index, ran)
    return got


def check_rank(src, w, h, index):
    want = Ref.run("rank", src, "width=%d,height=%d,index=%d" % (w, h, index))
    same(run_rank(src, w, h, index), want, "rank %dx%d[%d] on %s %s" % (w, h, index, src.shape, src.dtype))


# ---- rank against the reference

@pytest.mark.parametrize("window", WINDOWS, ids=lambda w: "%dx%d" % w)
def test_rank_windows(window):
    """Every window (they cross the reference's n > 10 and n > 90 route switches) x every index x every band count,
    uchar, on an image that IS the window, one pel larger, and one tile + 1."""
    w, h = window
    (tw, th), _ = tiles()
    for bands in BANDS:
        at = -(-tw // bands)
        for width, height in ((w, h), (w + 1, h + 1), (max(at + 1, w), max(th + 1, h))):
            src = noise(width, height, bands, np.uint8, 11 + bands)
            for index in indexes(w * h):
                check_rank(src, w, h, index)


@pytest.mark.parametrize("bands", BANDS)
def test_rank_sizes_round_the_tile(bands):
    """One window per kernel family on every width x height round the tile: T - 1, T, T + 1, 2 T + 5."""
    widths, heights = round_the_tile(tiles()[0], bands)
    for w, h, index in ((3, 3, 4), (5, 5, 12), (3, 3, 0), (4, 3, 11)):
        for width in widths:
            for height in heights:
                check_rank(noise(width, height, bands, np.uint8, 21 + bands), w, h, index)


@pytest.mark.parametrize("dtype", [np.uint16, np.int16, np.int32, np.float32, np.int8, np.uint32],
                         ids=lambda d: np.dtype(d).name)
def test_rank_formats(dtype):
    """The formats beside uchar (char and uint ride along: the kernels take them) on 3 x 3, 5 x 5 and 11 x 11 with
    every index, at one tile + 1.  Integer noise is full range, so signed formats cross zero."""
    (tw, th), _ = tiles()
    for bands in (1, 3):
        at = -(-tw // bands)
        for w, h in ((3, 3), (5, 5), (11, 11)):
            src = noise(max(at + 1, w), max(th + 1, h), bands, dtype, 31 + bands)
            if np.dtype(dtype).kind == "f":
                assert not np.isnan(src).any() and not np.signbit(src).any()
            for index in indexes(w * h):
                check_rank(src, w, h, index)


# ---- rank against a numpy model

def model_rank(src, w, h, index):
    """Edge-pad so that the window of (x, y) starts at (x - w // 2, y - h // 2), then the order statistic."""
    from numpy.lib.stride_tricks import sliding_window_view

    padded = np.pad(src, ((h // 2, h - 1 - h // 2), (w // 2, w - 1 - w // 2), (0, 0)), mode="edge")
    win = sliding_window_view(padded, (h, w), axis=(0, 1))
    flat = win.reshape(win.shape[:3] + (h * w,))
    return np.ascontiguousarray(np.partition(flat, index, axis=-1)[..., index])


def test_the_model_is_the_reference():
    for (width, height, bands, dtype, w, h, index) in ((61, 23, 3, np.uint8, 4, 3, 5), (40, 37, 1, np.int16, 7, 13, 45),
                                                     (33, 19, 4, np.float32, 2, 2, 1)):
        src = noise(width, height, bands, dtype, 41)
        want = Ref.run("rank", src, "width=%d,height=%d,index=%d" % (w, h, index))
        same(model_rank(src, w, h, index), want, "model %dx%d[%d]" % (w, h, index))


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float32], ids=lambda d: np.dtype(d).name)
def test_rank_sweep_against_the_model(dtype):
    """Odd image sizes, windows and band counts beside the lists above (2 and 5 bands, even windows, windows as
    large as the image in one direction), every kernel family."""
    sweep = [(1, 1, 1, 1, 1), (7, 5, 2, 7, 5), (19, 3, 5, 6, 3), (259, 9, 1, 9, 2), (87, 10, 3, 2, 9),
             (131, 17, 2, 15, 15), (53, 33, 5, 3, 3), (65, 7, 4, 8, 7), (300, 13, 3, 5, 5), (41, 41, 1, 31, 31)]
    for width, height, bands, w, h in sweep:
        src = noise(width, height, bands, dtype, 51 + bands)
        for index in indexes(w * h):
            same(run_rank(src, w, h, index), model_rank(src, w, h, index),
                 "%dx%dx%d rank %dx%d[%d]" % (width, height, bands, w, h, index))


@pytest.mark.parametrize("size", [3, 5, 7])
def test_median(size):
    src = noise(90, 37, 3, np.uint8, 61)
    im = Image.new_from_array(src)
    with gated() as g:
        got = im.median(size).numpy()
    assert {k for k in g.report if k.startswith("rank_")} == {rank_family(size, size, size * size // 2)}
    same(got, im.rank(size, size, size * size // 2).numpy(), "median %d" % size)
    same(got, Ref.run("rank", src, "width=%d,height=%d,index=%d" % (size, size, size * size // 2)),
         "median %d against the reference" % size)


# ---- morph against the reference

def disc(side):
    y, x = np.mgrid[0:side, 0:side]
    r = (side - 1) / 2.0
    return np.where((x - r) ** 2 + (y - r) ** 2 <= r * r + 0.5, 255.0, 128.0)


MASKS = {
    "full3": np.full((3, 3), 255.0),
    "cross3": np.array([[128, 255, 128], [255, 255, 255], [128, 255, 128]], float),
    "mixed": np.array([[0, 255, 128, 255, 0], [128, 128, 255, 0, 128], [255, 0, 0, 128, 255]], float),
    "even2x2": np.array([[255, 0], [128, 255]], float),
    "even4x3": np.array([[255, 128, 0, 255], [128, 255, 255, 128], [0, 128, 128, 255]], float),
    "row1x5": np.array([[255, 128, 255, 0, 255]], float),
    "column5x1": np.array([[255], [0], [128], [255], [255]], float),
    "all128": np.full((3, 3), 128.0),
    "disc31": disc(31),
}


def blobs(w, h, bands, seed):
    """0 / 255 shapes: noise thresholded after a blur, so that erosion and dilation have borders to move."""
    a = noise(w + 8, h + 8, bands, np.uint8, seed).astype(np.int32)
    s = sum(a[dy:dy + h, dx:dx + w] for dy in range(0, 9, 2) for dx in range(0, 9, 2))
    return np.where(s > 25 * 128, 255, 0).astype(np.uint8)


def run_morph(src, mask, op):
    with gated() as g:
        got = Image.new_from_array(src).morph(mask, op).numpy()
    ran = {k: n for k, (n, _) in g.report.items() if k.startswith("morph_")}
    assert ran == {"morph_" + op: 1}, (op, ran)
    return got


def check_morph(src, mask, op, what):
    want = Ref.run_mask("morph", src, mask, args="morph=" + op)
    got = run_morph(src, mask, op)
    assert got.dtype == np.uint8
    same(got, want, "%s %s on %s %s" % (op, what, src.shape, src.dtype))


@pytest.mark.parametrize("name", sorted(MASKS))
def test_morph_masks(name):
    """Every mask x erode / dilate x 0 / 255 blobs and full-range byte noise (only noise shows that the operations
    are bitwise) x every band count, on an image of one tile + 1 and on one smaller than the mask's rows."""
    mask = MASKS[name]
    _, (tw, th) = tiles()
    for bands in BANDS:
        at = -(-tw // bands)
        for width, height in ((at + 1, th + 1), (7, 2)):
            for src in (blobs(width, height, bands, 71 + bands), noise(width, height, bands, np.uint8, 75 + bands)):
                for op in ("erode", "dilate"):
                    check_morph(src, mask, op, name)


def test_morph_all128_is_constant():
    src = noise(40, 9, 3, np.uint8, 79)
    assert (run_morph(src, MASKS["all128"], "dilate") == 0).all()
    assert (run_morph(src, MASKS["all128"], "erode") == 255).all()


@pytest.mark.parametrize("bands", BANDS)
def test_morph_sizes_round_the_tile(bands):
    widths, heights = round_the_tile(tiles()[1], bands)
    for width in widths:
        for height in heights:
            src = noise(width, height, bands, np.uint8, 81 + bands)
            check_morph(src, MASKS["mixed"], "erode", "mixed")
            check_morph(src, MASKS["even4x3"], "dilate", "even4x3")


@pytest.mark.parametrize("dtype", [np.uint16, np.float32], ids=lambda d: np.dtype(d).name)
def test_morph_casts_to_uchar(dtype):
    """Other formats are vips_cast to uchar first: values past both ends of 0 .. 255, fractions."""
    src = noise(130, 21, 3, dtype, 91)
    if np.dtype(dtype).kind == "f":
        src = ((src - np.float32(64)) * np.float32(2)).astype(np.float32)
    else:
        src = (src % 400).astype(dtype)
    for op in ("erode", "dilate"):
        check_morph(src, MASKS["cross3"], op, "cross3")
        check_morph(src, MASKS["mixed"], op, "mixed")


# ---- the region form

RECTS = ((20, 15, 40, 30), (0, 0, 17, 9), (70, 55, 20, 15), (0, 60, 90, 10), (85, 0, 5, 70))


def region_pair(src, rect, half, out_dtype):
    """An input window that only just covers what the output rect (left, top, w, h) reads, and the output."""
    H, W = src.shape[:2]
    left, top, w, h = rect
    (ax, bx), (ay, by) = half
    x0, y0 = max(left - ax, 0), max(top - ay, 0)
    x1, y1 = min(left + w + bx, W), min(top + h + by, H)
    win = Image.new_from_array(np.ascontiguousarray(src[y0:y1, x0:x1]))
    rin = win.region()
    rin.left, rin.top, rin.im_width, rin.im_height = x0, y0, W, H
    out = Image.new_from_array(np.zeros((h, w, src.shape[2]), out_dtype))
    rout = out.region()
    rout.left, rout.top, rout.im_width, rout.im_height = left, top, W, H
    return win, rin, out, rout


@pytest.mark.parametrize("case", [(np.uint8, 3, 3, 4), (np.uint8, 6, 5, 0), (np.uint16, 5, 4, 7), (np.float32, 7, 3, 20)],
                         ids=lambda c: "%s-%dx%d-%d" % (np.dtype(c[0]).name, c[1], c[2], c[3]))
def test_rank_region_form(case):
    """An output rect strictly inside the image and rects touching every edge, from an input window that only just
    covers them, against the same rect of the whole-image result."""
    dtype, w, h, index = case
    src = noise(90, 70, 2, dtype, 101)
    whole = run_rank(src, w, h, index)
    half = ((w // 2, w - 1 - w // 2), (h // 2, h - 1 - h // 2))
    for rect in RECTS:
        win, rin, out, rout = region_pair(src, rect, half, dtype)
        with gated() as g:
            _ffi.check(lib.vips_hip_rank_gen(ctypes.byref(rin), ctypes.byref(rout), w, h, index))
            got = out.numpy()
        assert rank_family(w, h, index) in g.report
        left, top, rw, rh = rect
        same(got, np.ascontiguousarray(whole[top:top + rh, left:left + rw]), "rank region %r" % (rect,))
    # a window that does not hold the halo
    win, rin, out, rout = region_pair(src, RECTS[0], ((0, 0), (0, 0)), dtype)
    lib.vips_hip_error_clear()
    assert lib.vips_hip_rank_gen(ctypes.byref(rin), ctypes.byref(rout), w, h, index) == -1
    assert "rank: input region too small" in _ffi.error_buffer()
    lib.vips_hip_error_clear()


@pytest.mark.parametrize("name,op,dtype", [("mixed", "erode", np.uint8), ("even4x3", "dilate", np.uint8),
                                           ("cross3", "dilate", np.uint16)])
def test_morph_region_form(name, op, dtype):
    mask = np.ascontiguousarray(MASKS[name])
    mh, mw = mask.shape
    src = noise(90, 70, 3, dtype, 103)
    whole = run_morph(src, mask, op)
    half = ((mw // 2, mw - 1 - mw // 2), (mh // 2, mh - 1 - mh // 2))
    for rect in RECTS:
        win, rin, out, rout = region_pair(src, rect, half, np.uint8)
        with gated() as g:
            _ffi.check(lib.vips_hip_morph_gen(ctypes.byref(rin), ctypes.byref(rout),
                                              mask.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), mw, mh,
                                              libvips_amd.image.MORPHOLOGIES[op]))
            got = out.numpy()
        assert "morph_" + op in g.report
        left, top, rw, rh = rect
        same(got, np.ascontiguousarray(whole[top:top + rh, left:left + rw]), "morph region %r" % (rect,))


def test_need_rule():
    top, rows = ctypes.c_int(), ctypes.c_int()
    for window, at, n in ((3, 16, 16), (4, 0, 5), (31, 100, 1), (1, 7, 9)):
        lib.vips_hip_rank_need(window, at, n, ctypes.byref(top), ctypes.byref(rows))
        assert (top.value, rows.value) == (at - window // 2, n + window - 1)


# ---- refusals and errors

def test_errors_and_refusals():
    im = Image.new_from_array(noise(40, 30, 3, np.uint8, 111))
    with pytest.raises(VipsHipError, match="rank: window too large"):
        im.rank(41, 3, 0)
    with pytest.raises(VipsHipError, match="rank: window too large"):
        im.rank(3, 31, 0)
    with pytest.raises(VipsHipError, match="rank: index out of range"):
        im.rank(3, 3, 9)
    with pytest.raises(VipsHipError, match="rank: index out of range"):
        im.rank(3, 3, -1)
    with pytest.raises(VipsHipError, match=r"morph: bad mask element \(7\.000000 should be 0, 128 or 255\)"):
        im.morph([[255, 7, 128]], "erode")
    # the reference says the same three things
    src = noise(40, 30, 3, np.uint8, 111)
    with pytest.raises(RuntimeError, match="window too large"):
        Ref.run("rank", src, "width=41,height=3,index=0")
    with pytest.raises(RuntimeError, match="index out of range"):
        Ref.run("rank", src, "width=3,height=3,index=9")
    with pytest.raises(RuntimeError, match=r"bad mask element \(7\.000000 should be 0, 128 or 255\)"):
        Ref.run_mask("morph", src, np.array([[255.0, 7.0, 128.0]]), args="morph=erode")
    # what the device does not take is refused by name: no other path runs it
    with pytest.raises(VipsHipError, match="rank: double images"):
        Image.new_from_array(noise(40, 30, 1, np.float64, 112)).rank(3, 3, 4)
    big = Image.new_from_array(noise(300, 300, 1, np.uint8, 113))
    with pytest.raises(VipsHipError, match="rank: a 300 x 300 window .* LDS"):
        big.rank(300, 300, 5)
    side = lib.vips_hip_rank_step(4)
    assert side >= 31
    with pytest.raises(VipsHipError, match="morph: a %d x 3 mask" % (side + 1)):
        big.morph(np.full((3, side + 1), 255.0), "dilate")
    with pytest.raises(VipsHipError, match="morph: .* LDS"):
        Image.new_from_array(noise(40, 8, 90, np.uint8, 114)).morph(np.full((side, side), 255.0), "dilate")
    # and the largest ones it does take run
    same(big.rank(31, 31, 480).numpy(), model_rank(noise(300, 300, 1, np.uint8, 113), 31, 31, 480), "31 x 31")


# ---- the libvips module

@needs_module
@pytest.mark.parametrize("strips", [False, True], ids=["whole", "strips"])
def test_module_rank_and_morph(strips):
    """rank_hip and morph_hip make the built-in operations' pixels, whole and strip by strip (a small
    $VIPS_HIP_BUDGET, as tests/test_module.py), a wide-range ushort input to morph_hip included."""
    Ref.load_module()
    module = ctypes.CDLL(helpers.MODULE_LIB)
    height = 900 if strips else 60
    src = helpers.lcg_image(500, height, 3, np.uint8, 121)
    wide = (helpers.lcg_image(500, height, 1, np.uint16, 122) % 300).astype(np.uint16)
    if strips:
        os.environ["VIPS_HIP_BUDGET"] = "300k"
    before = module.vips_hip_module_strips_done()
    try:
        for args in ("width=3,height=3,index=4", "width=5,height=9,index=0", "width=4,height=7,index=13"):
            same(Ref.run("rank_hip", src, args), Ref.run("rank", src, args), "rank_hip " + args)
        for name, op in (("cross3", "erode"), ("mixed", "dilate"), ("disc31", "dilate")):
            same(Ref.run_mask("morph_hip", src, MASKS[name], args="morph=" + op),
                 Ref.run_mask("morph", src, MASKS[name], args="morph=" + op), "morph_hip %s %s" % (name, op))
        same(Ref.run_mask("morph_hip", wide, MASKS["mixed"], args="morph=erode"),
             Ref.run_mask("morph", wide, MASKS["mixed"], args="morph=erode"), "morph_hip ushort")
    finally:
        if strips:
            del os.environ["VIPS_HIP_BUDGET"]
    if strips:
        assert module.vips_hip_module_strips_done() - before >= 7 * 2, "not strip-mined"


@needs_module
def test_module_errors_are_the_originals():
    Ref.load_module()
    src = noise(40, 30, 3, np.uint8, 111)
    with pytest.raises(RuntimeError, match="rank_hip: window too large"):
        Ref.run("rank_hip", src, "width=41,height=3,index=0")
    with pytest.raises(RuntimeError, match="rank_hip: index out of range"):
        Ref.run("rank_hip", src, "width=3,height=3,index=9")
    with pytest.raises(RuntimeError, match=r"morph_hip: bad mask element"):
        Ref.run_mask("morph_hip", src, np.array([[255.0, 7.0, 128.0]]), args="morph=erode")
