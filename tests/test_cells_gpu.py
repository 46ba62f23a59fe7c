"""GPU parity: sheets and tiles on the device -- vips_arrayjoin, vips_replicate, vips_wrap, vips_grid (libvips_amd/csrc/
cells.hip, ops_cells.cpp) and vips_zoom / vips_subsample as whole-image calls.

All of it is data movement, so every comparison is np.array_equal on values, dtype and shape (and the interpretation
where the reference sets one); nothing has a tolerance.  One-image operations reach the reference through Ref.run,
vips_arrayjoin through its command line, which pins the numpy model of tests/cells_model.py; the sweeps then run against
the model.  Every case asserts by the gate report which kernel ran and that it was launched once.
Runs on the CPU too, on host fibers (tests/test_emul_cells.py)."""
import ctypes
import os

import numpy as np
import pytest

import libvips_amd
from libvips_amd import Image, VipsHipError, _ffi
from tests import cells_model as model
from tests import helpers
from tests.helpers import Ref

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not helpers.have_ref(), reason="oracle/_ref not built")]

lib = _ffi.lib
INTERP = helpers.INTERP
# pel size -> (dtype, bands)
PELS = {1: (np.uint8, 1), 2: (np.uint16, 1), 3: (np.uint8, 3), 4: (np.uint8, 4), 6: (np.uint16, 3), 8: (np.uint16, 4),
        12: (np.float32, 3), 16: (np.float32, 4), 24: (np.float64, 3), 32: (np.float64, 4)}
SENTINEL = 0xA5


@pytest.fixture(scope="module", autouse=True)
def _init():
    libvips_amd.init(0)


class gated(object):
    """with gated() as g: ...; g.ran: {gate name: launches} of this feature's kernels that ran inside."""

    def __enter__(self):
        lib.vips_hip_gate_reset()
        lib.vips_hip_gate_enable(1)
        self.ran = None
        return self

    def __exit__(self, *exc):
        try:
            if exc[0] is None:
                self.ran = {k: n for k, (n, _) in libvips_amd.gate_report().items()
                            if k.startswith("cells_") or k in ("zoom", "subsample")}
        finally:
            lib.vips_hip_gate_enable(0)
            lib.vips_hip_gate_reset()
        return False


class general_kernel(object):
    """The one-pel-a-lane kernel for everything inside (the library reads the variable at every dispatch)."""

    def __init__(self, on=True):
        self.on = on

    def __enter__(self):
        if self.on:
            os.environ["VIPS_HIP_NO_CELLS_STREAM"] = "1"

    def __exit__(self, *exc):
        os.environ.pop("VIPS_HIP_NO_CELLS_STREAM", None)
        return False


def same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), what


def noise(w, h, dtype, bands, seed):
    return np.ascontiguousarray(helpers.lcg_image(w, h, bands, dtype, seed))


def ink_of(background, bands, dtype):
    """vips__vector_to_ink through the library (pinned to the reference in tests/test_canvas_host.py and, here, by
    test_the_arrayjoin_model_is_the_reference)."""
    bg = np.atleast_1d(np.asarray(background if background is not None else 0, np.float64))
    out = np.zeros(bands, dtype)
    _ffi.check(lib.vips_hip_vector_to_ink(bg.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), len(bg), bands,
                                          helpers.DTYPE_FORMATS[np.dtype(dtype)], out.ctypes.data))
    return out


def expect_kernel(kernel, pel, on_dwords=True):
    """The gate report of one launch: the streaming kernel where it is asked for, takes the pel size and rows start on
    dwords; the one-pel-a-lane kernel otherwise."""
    streams = kernel == "stream" and lib.vips_hip_cells_step(1, pel) != 0 and on_dwords
    return {"cells_stream" if streams else "cells_general": 1}


def step_widths(pel):
    """Cell widths in pels whose rows are 1, 15, 16, 17, 47, 48, 49 bytes (rounded up to whole pels) and one wave's worth
    of the streaming kernel's groups - 1 / + 0 / + 1 pel."""
    group = lib.vips_hip_cells_step(1, pel) or 16
    wave = 64 * group // pel if group % pel == 0 else 64
    return sorted({-(-n // pel) for n in (1, 15, 16, 17, 47, 48, 49)} | {wave - 1, wave, wave + 1})


def dev_arrayjoin(arrays, interps=None, **kw):
    """-> (array, interpretation, gate report) of Image.arrayjoin."""
    images = [Image.new_from_array(a, interps[i] if interps else 0) for i, a in enumerate(arrays)]
    with gated() as g:
        out = Image.arrayjoin(images, **kw)
    return out.numpy(), lib.vips_hip_image_get_interpretation(out._h), g.ran


def model_arrayjoin(arrays, background=None, **kw):
    n_background = len(np.atleast_1d(background)) if background is not None else 1
    images = model.alike(arrays, n_background)
    return model.arrayjoin(images, ink_of(background, images[0].shape[2], images[0].dtype), **kw)


# ---------------------------------------------------------------- 1. the model is the reference

def check_against_the_reference(tmp_path, arrays, interps, what, **kw):
    want, want_interp = model.ref_arrayjoin(tmp_path, list(zip(arrays, interps)), model.cli_options(**kw))
    same(model_arrayjoin(arrays, **kw), want, ("model", what, kw))
    got, interp, ran = dev_arrayjoin(arrays, interps, **kw)
    same(got, want, ("device", what, kw))
    assert interp == want_interp, (what, kw, interp, want_interp)
    cells = {k: v for k, v in ran.items() if k.startswith("cells_")}  # (vips__bandup is a zoom of the elements)
    assert sum(cells.values()) == 1, ran


@pytest.mark.parametrize("n", [1, 2, 5, 7])
def test_the_arrayjoin_model_is_the_reference(tmp_path, n):
    """n images of different sizes across 3, with and without a shim, every halign x valign."""
    arrays = [noise(4 + (3 * i) % 5, 3 + (2 * i) % 4, np.uint8, 3, 11 + i) for i in range(n)]
    interps = [INTERP["srgb"]] * n
    for shim in (0, 2):
        for halign in model.ALIGNS:
            for valign in model.ALIGNS:
                check_against_the_reference(tmp_path, arrays, interps, n, across=3, shim=shim, halign=halign, valign=valign,
                                            background=[10, 200, 30] if shim else None)


def test_the_model_is_the_reference_for_bands_and_formats(tmp_path):
    """A three-element background on one-band images (the bands follow the background); uchar + ushort + float; one band
    + three bands, the tag of the image with the most bands; a vector of the wrong length."""
    bw, srgb, rgb16 = INTERP["b-w"], INTERP["srgb"], INTERP["rgb16"]
    one = [noise(5, 4, np.uint8, 1, 21), noise(3, 6, np.uint8, 1, 22), noise(6, 2, np.uint8, 1, 23)]
    check_against_the_reference(tmp_path, one, [bw] * 3, "background of three", across=2, shim=1, background=[9, 99, 199])
    mixed = [noise(5, 4, np.uint8, 3, 24), noise(4, 5, np.uint16, 3, 25), noise(6, 3, np.float32, 3, 26)]
    check_against_the_reference(tmp_path, mixed, [srgb, rgb16, srgb], "formats", across=2, halign="centre", background=300.5)
    bands = [noise(5, 4, np.uint8, 1, 27), noise(4, 5, np.uint8, 3, 28), noise(3, 3, np.uint16, 1, 29)]
    check_against_the_reference(tmp_path, bands, [bw, srgb, bw], "bands", across=3, shim=3, valign="high")
    check_against_the_reference(tmp_path, bands[::-1], [bw, srgb, bw], "bands, the first banded up", across=2)
    with pytest.raises(RuntimeError, match="vector must have 1 or 3 elements"):
        model.ref_arrayjoin(tmp_path, [(bands[1], srgb), (mixed[0], srgb)], ["--background", "1 2"])
    lib.vips_hip_error_clear()
    with pytest.raises(VipsHipError, match="vector must have 1 or 3 elements"):
        Image.arrayjoin([Image.new_from_array(bands[1]), Image.new_from_array(mixed[0])], background=[1, 2])
    # ... which nobody looks at where every image fills its rect: each vips_embed is then a copy
    want, _ = model.ref_arrayjoin(tmp_path, [(bands[1], srgb)] * 2, ["--background", "1 2", "--across", "1"])
    got, _, _ = dev_arrayjoin([bands[1]] * 2, [srgb] * 2, background=[1, 2], across=1)
    same(got, want, "a background of the wrong length that is never painted")
    with pytest.raises(RuntimeError, match="not one band or 3 bands"):
        model.ref_arrayjoin(tmp_path, [(bands[1], srgb), (noise(3, 3, np.uint8, 2, 30), 0)])
    with pytest.raises(VipsHipError, match="arrayjoin: not one band or 3 bands"):
        Image.arrayjoin([Image.new_from_array(bands[1]), Image.new_from_array(noise(3, 3, np.uint8, 2, 30))])


def test_anchors():
    """Three one-band images of constants: what the reference was seen to make of them."""
    ims = [np.full((2, 3, 1), v, np.uint8) for v in (1, 2, 3)]
    got, _, ran = dev_arrayjoin(ims, across=2, shim=1, background=9)
    assert got[:, :, 0].tolist() == [[1, 1, 1, 9, 2, 2, 2], [1, 1, 1, 9, 2, 2, 2], [9] * 7, [3, 3, 3, 9, 9, 9, 9], [3, 3, 3, 9, 9, 9, 9]]
    assert ran == {"cells_general": 1}, ran


# ---------------------------------------------------------------- 2. the sweep: both kernels, ten pel sizes

@pytest.mark.parametrize("kernel", ["stream", "general"])
@pytest.mark.parametrize("pel", sorted(PELS))
def test_arrayjoin_sweep(pel, kernel):
    """Six images four across (the last row is filled by the clamp) in boxes of every width of step_widths(): the images'
    rows are whole dwords and the boxes crop or pad them, so that an image's edge, a shim and a cell's edge fall anywhere
    in a group.  24- and 32-byte pels take the one-pel-a-lane kernel."""
    dtype, bands = PELS[pel]
    background = [10, 200, 30, 77][:bands] if bands > 1 else 200
    for cw in step_widths(pel):
        widths = [max(4, cw // 4 * 4), (cw + 3) // 4 * 4, 4, cw // 4 * 4 + 8, max(4, cw // 8 * 4), (cw + 3) // 4 * 4]
        arrays = [noise(w, 2 + i % 2, dtype, bands, 100 + cw + i) for i, w in enumerate(widths)]
        for shim, halign in ((0, "low"), (4, "centre"), (0, "high")):
            kw = dict(across=4, shim=shim, halign=halign, valign="centre", hspacing=cw, background=background)
            with general_kernel(kernel == "general"):
                got, _, ran = dev_arrayjoin(arrays, **kw)
            assert ran == expect_kernel(kernel, pel), (ran, pel, cw, shim)
            same(got, model_arrayjoin(arrays, **kw), (kernel, pel, cw, shim, halign))


@pytest.mark.parametrize("kernel", ["stream", "general"])
def test_rows_off_dwords_take_the_general_kernel(kernel):
    """A 3-band uchar sheet whose width is no multiple of 4 (and images whose rows are not), ushort rows of odd length."""
    for pel, w in ((3, 5), (3, 7), (2, 3), (1, 6), (6, 3)):
        dtype, bands = PELS[pel]
        arrays = [noise(w, 3, dtype, bands, 200 + i) for i in range(4)]
        with general_kernel(kernel == "general"):
            got, _, ran = dev_arrayjoin(arrays, across=3, shim=1)
        assert ran == {"cells_general": 1}, (ran, pel, w)
        same(got, model_arrayjoin(arrays, across=3, shim=1), (pel, w))
    # the images' rows on dwords, the sheet's not
    arrays = [noise(4, 3, np.uint8, 3, 210 + i) for i in range(3)]
    with general_kernel(kernel == "general"):
        got, _, ran = dev_arrayjoin(arrays, across=3, shim=1)
    assert ran == {"cells_general": 1}, ran
    same(got, model_arrayjoin(arrays, across=3, shim=1), "sheet off dwords")


@pytest.mark.parametrize("kernel", ["stream", "general"])
def test_groups_that_straddle(kernel):
    """Image, shim, image and shim inside one 16-byte group; cells narrower than a group; a group over two cells."""
    for pel in (1, 2, 4):
        dtype, bands = PELS[pel]
        w = 4 // pel
        arrays = [noise(w, 2, dtype, bands, 220 + i) for i in range(11)]
        for shim in (4 // pel, 8 // pel):
            kw = dict(across=4, shim=shim, background=[7, 8, 9, 10][:bands])
            with general_kernel(kernel == "general"):
                got, _, ran = dev_arrayjoin(arrays, **kw)
            assert ran == expect_kernel(kernel, pel), ran
            same(got, model_arrayjoin(arrays, **kw), (pel, shim))


# ---------------------------------------------------------------- regions: windows of larger frames

def upload_frame(frame):
    """A (rows, stride) uint8 array in HBM."""
    return Image.new_from_array(np.ascontiguousarray(frame)[:, :, None])


def gen_in_frames(call, src, out_size, in_window=None, out_rect=None, margin=4):
    """A region function with the input and the output as windows of larger frames whose rows start on dwords (margin *
    pel a multiple of 4) or anywhere (margin 1 .. 3 with an odd pel); the output frame's bytes outside the window must
    stay as they were.  call(rin, rout) runs it; in_window / out_rect: (left, top, width, height) of the image that the
    input frame holds / of the output that is made; out_size the whole output's (width, height)."""
    h, w, b = src.shape
    pel = b * src.dtype.itemsize
    il, it, iw, ih = in_window or (0, 0, w, h)
    ol, ot, ow, oh = out_rect or (0, 0) + tuple(out_size)
    raw = np.ascontiguousarray(src[it:it + ih, il:il + iw]).view(np.uint8).reshape(ih, iw * pel)
    istride = (margin * pel + iw * pel + 5 + 3) // 4 * 4
    fin = np.full((ih + 2, istride), 0x3C, np.uint8)
    fin[1:1 + ih, margin * pel:margin * pel + iw * pel] = raw
    ostride = (margin * pel + ow * pel + 7 + 3) // 4 * 4
    fout = np.full((oh + 2, ostride), SENTINEL, np.uint8)
    din, dout = upload_frame(fin), upload_frame(fout)
    fmt = helpers.DTYPE_FORMATS[src.dtype]
    rin = _ffi.Region(din.data_ptr + istride + margin * pel, il, it, iw, ih, w, h, b, fmt, istride)
    rout = _ffi.Region(dout.data_ptr + ostride + margin * pel, ol, ot, ow, oh, out_size[0], out_size[1], b, fmt, ostride)
    _ffi.check(call(ctypes.byref(rin), ctypes.byref(rout)))
    back = dout.numpy()[:, :, 0]
    got = back[1:1 + oh, margin * pel:margin * pel + ow * pel].copy()
    back[1:1 + oh, margin * pel:margin * pel + ow * pel] = SENTINEL
    assert (back == SENTINEL).all(), "bytes outside the output window were written"
    return np.ascontiguousarray(got).view(src.dtype).reshape(oh, ow, b)


@pytest.mark.parametrize("kernel", ["stream", "general"])
@pytest.mark.parametrize("pel", sorted(PELS))
def test_replicate_sweep(pel, kernel):
    """Periods of every width of step_widths(), their rows starting on dwords inside frames: a source group starts
    anywhere in its row, a group holds one period's end and the next one's start."""
    dtype, bands = PELS[pel]
    for cw in step_widths(pel):
        src = noise(cw, 2, dtype, bands, 300 + cw)
        for x0, y0 in ((0, 0), (cw // 2, 1), (cw, 2)):
            size = (3 * cw + 1, 5)
            with general_kernel(kernel == "general"), gated() as g:
                got = gen_in_frames(lambda ri, ro: lib.vips_hip_replicate_gen(x0, y0, ri, ro), src, size)
            assert g.ran == expect_kernel(kernel, pel), (g.ran, pel, cw)
            same(got, model.replicate(src, 0, 0, x0, y0, *size), (kernel, pel, cw, x0, y0))


@pytest.mark.parametrize("kernel", ["stream", "general"])
def test_tiny_images_replicated(kernel):
    """1 x 1 and 2 x 3 pel images 40 x 9 times: cells narrower than a group.  Whole images (rows of one or two pels start
    anywhere: the one-pel-a-lane kernel unless a row is whole dwords) and in frames (rows on dwords: the streaming one)."""
    for pel in (1, 3, 4, 12):
        dtype, bands = PELS[pel]
        for w, h in ((1, 1), (2, 3)):
            src = noise(w, h, dtype, bands, 400 + w)
            want = model.replicate(src, 40, 9)
            with general_kernel(kernel == "general"), gated() as g:
                got = Image.new_from_array(src).replicate(40, 9).numpy()
            assert g.ran == expect_kernel(kernel, pel, (w * pel) % 4 == 0), (g.ran, pel, w)
            same(got, want, (kernel, pel, w, h))
            with general_kernel(kernel == "general"), gated() as g:
                got = gen_in_frames(lambda ri, ro: lib.vips_hip_replicate_gen(0, 0, ri, ro), src, (40 * w, 9 * h))
            assert g.ran == expect_kernel(kernel, pel), (g.ran, pel, w)
            same(got, want, ("frames", kernel, pel, w, h))


# ---------------------------------------------------------------- 3. the clamp and the stretch

MANY = {}


def many_images(pel, n, across):
    """n images of 5 x 3 .. 7 x 5 pels on the device and the sheet the model makes of them: made once, shared by the
    two kernels' cases."""
    if (pel, n) not in MANY:
        dtype, bands = PELS[pel]
        arrays = [noise(5 + i % 3, 3 + (i // 3) % 3, dtype, bands, 500 + i) for i in range(n)]
        kw = dict(across=across, shim=1, halign="centre", valign="high", background=[1, 2, 3, 4][:bands])
        MANY[pel, n] = ([Image.new_from_array(a) for a in arrays], kw, model_arrayjoin(arrays, **kw))
    return MANY[pel, n]


@pytest.mark.parametrize("kernel", ["stream", "general"])
def test_the_clamp_and_the_stretch(kernel):
    """n = 5 across 3, and 301 images of 5 x 3 .. 7 x 5 pels across 17: a table larger than a block reads at once, a last
    row that the last image's rect fills.  (Rows of 5 .. 7 three-byte pels are no whole dwords.)"""
    for pel, n, across in ((4, 5, 3), (3, 5, 3), (4, 301, 17)):
        images, kw, want = many_images(pel, n, across)
        with general_kernel(kernel == "general"), gated() as g:
            got = Image.arrayjoin(images, **kw).numpy()
        assert g.ran == expect_kernel(kernel, pel, pel == 4), g.ran
        assert want.shape[1] == across * 8 - 1 and n % across != 0  # boxes of 7 and a shim; a last row with cells to fill
        same(got, want, (kernel, pel, n))


# ---------------------------------------------------------------- 4. cropping

@pytest.mark.parametrize("kernel", ["stream", "general"])
def test_boxes_smaller_than_the_images(tmp_path, kernel):
    """hspacing / vspacing smaller than some images and larger than others, every align: offsets of every sign.  One
    case of each align goes to the reference's command line too."""
    arrays = [noise(w, h, np.uint8, 4, 600 + w) for w, h in ((12, 9), (4, 3), (8, 6), (16, 2), (5, 11))]
    for halign in model.ALIGNS:
        for valign in model.ALIGNS:
            kw = dict(across=2, shim=2, halign=halign, valign=valign, hspacing=8, vspacing=6, background=[5, 6, 7, 8])
            with general_kernel(kernel == "general"):
                got, _, ran = dev_arrayjoin(arrays, **kw)
            assert ran == expect_kernel(kernel, 4), ran
            want = model_arrayjoin(arrays, **kw)
            same(got, want, (kernel, halign, valign))
            if halign == valign:
                ref, _ = model.ref_arrayjoin(tmp_path, [(a, INTERP["srgb"]) for a in arrays], model.cli_options(**kw))
                same(want, ref, ("model", halign, valign))


# ---------------------------------------------------------------- 5. replicate, wrap, grid against the reference

def both(fn_dev, fn_ref, what, kernels=("cells_stream", "cells_general")):
    """The library's result and the reference's: equal images (and interpretations), one launch of one of `kernels`; or
    both an error with the reference's words (what follows its nickname) in the library's message."""
    try:
        want, interpretation = fn_ref()
    except RuntimeError as e:
        words = str(e).strip().splitlines()[-1].split(": ")[-1]
        lib.vips_hip_error_clear()
        with pytest.raises(VipsHipError) as info:
            fn_dev()
        assert words in str(info.value), (what, str(e), str(info.value))
        return None
    with gated() as g:
        got = fn_dev()
    if kernels:
        assert sum(g.ran.values()) == 1 and set(g.ran) <= set(kernels), (what, g.ran)
    assert lib.vips_hip_image_get_interpretation(got._h) == interpretation, (what, "interpretation")
    same(got.numpy(), want, what)
    return got


SOURCES = [(np.uint8, 3, "srgb"), (np.uint16, 4, "rgb16"), (np.float64, 1, "b-w"), (np.float64, 4, "srgb")]


@pytest.mark.parametrize("kernel", ["stream", "general"])
def test_replicate_wrap_grid_against_the_reference(kernel):
    for dtype, bands, interp in SOURCES:
        code = INTERP[interp]
        src = noise(8, 60, dtype, bands, 700)
        im = Image.new_from_array(src, interp)
        with general_kernel(kernel == "general"):
            for across, down in ((1, 1), (3, 2), (1, 4), (5, 1)):
                both(lambda: im.replicate(across, down),
                     lambda: Ref.run_interp("replicate", src, "across=%d,down=%d" % (across, down), interpretation=code),
                     ("replicate", dtype, across, down))
            # the defaults, negative, beyond the image, a multiple of the width (x' is then the width itself), zero
            for x, y in ((None, None), (3, None), (-3, -7), (8, 60), (16, 0), (0, 0), (-8, 120), (11, -61), (100, 1000)):
                args = ",".join("%s=%d" % kv for kv in (("x", x), ("y", y)) if kv[1] is not None)
                both(lambda: im.wrap(x, y), lambda: Ref.run_interp("wrap", src, args, interpretation=code), ("wrap", dtype, x, y))
            for tile_height, across, down in ((60, 1, 1), (20, 1, 3), (20, 3, 1), (5, 3, 4), (1, 3, 20), (1, 4, 15), (5, 4, 3),
                                              (7, 3, 4), (5, 3, 3), (61, 1, 1)):
                both(lambda: im.grid(tile_height, across, down),
                     lambda: Ref.run_interp("grid", src, "tile_height=%d,across=%d,down=%d" % (tile_height, across, down),
                                            interpretation=code), ("grid", dtype, tile_height, across, down))


def test_wrap_origins():
    """wrap.c:86-91 in numbers: a positive multiple of the size gives the size itself, a negative one zero."""
    assert [model.wrap_origin(8, v) for v in (0, 8, 16, -8, 3, -3, 11, -11)] == [8, 8, 8, 0, 5, 3, 5, 3]
    src = noise(8, 5, np.uint8, 4, 710)
    im = Image.new_from_array(src)
    for x, y in ((0, 0), (8, 5), (16, -10), (3, -2), (-11, 7)):
        with gated() as g:
            got = im.wrap(x, y).numpy()
        assert g.ran == {"cells_stream": 1}, g.ran
        same(got, model.replicate(src, 1, 1, model.wrap_origin(8, x), model.wrap_origin(5, y), 8, 5), (x, y))


# ---------------------------------------------------------------- 6. zoom, subsample

def test_zoom_and_subsample_against_the_reference():
    """(Both name their image argument "input": model.ref_input is Ref.run_interp with that name.)"""
    for dtype, bands, interp in ((np.uint8, 3, "srgb"), (np.float64, 1, "b-w")):
        code = INTERP[interp]
        src = noise(23, 17, dtype, bands, 800)
        im = Image.new_from_array(src, interp)
        for xfac, yfac in ((1, 1), (2, 2), (3, 5)):
            copy = (xfac, yfac) == (1, 1)  # vips_image_write: no kernel of this family
            both(lambda: im.zoom(xfac, yfac), lambda: model.ref_input("zoom", src, "xfac=%d,yfac=%d" % (xfac, yfac), code),
                 ("zoom", dtype, xfac, yfac), () if copy else ("zoom",))
            for point in (False, True):
                args = "xfac=%d,yfac=%d" % (xfac, yfac) + (",point=true" if point else "")
                both(lambda: im.subsample(xfac, yfac, point=point), lambda: model.ref_input("subsample", src, args, code),
                     ("subsample", dtype, xfac, yfac, point), () if copy else ("subsample",))
        both(lambda: im.subsample(24, 1), lambda: model.ref_input("subsample", src, "xfac=24,yfac=1"), "shrunk")
        both(lambda: im.subsample(2, 18), lambda: model.ref_input("subsample", src, "xfac=2,yfac=18"), "shrunk")
        # (the largest factor the reference's arguments take: a side of more than INT_MAX / 2 needs 108 pels)
        big = noise(120, 110, dtype, bands, 801)
        for xfac, yfac in ((10000000, 1), (1, 10000000)):
            both(lambda: Image.new_from_array(big).zoom(xfac, yfac),
                 lambda: model.ref_input("zoom", big, "xfac=%d,yfac=%d" % (xfac, yfac)), "zoom too large")
    lib.vips_hip_error_clear()
    with pytest.raises(VipsHipError, match="zoom: zoom factors too large"):
        Image.new_from_array(noise(120, 8, np.uint8, 1, 802)).zoom(10000000, 1)
    with pytest.raises(VipsHipError, match="subsample: image has shrunk to nothing"):
        Image.new_from_array(noise(8, 8, np.uint8, 1, 802)).subsample(9, 1)


# ---------------------------------------------------------------- 6a. the capped grids' second turn

@pytest.mark.parametrize("pel", [4, 3])
def test_cells_stream_second_turn(tmp_path, pel):
    """A sheet of more 16-byte (RGBA) / 48-byte (RGB) groups than the capped grid has lanes, two cells across with a shim
    between them: the lanes' second group lies in the last row of cells, which holds a cell's edges, the shim, an image's
    bottom edge inside its box and the box no image fills; every row of the sheet ends in a ragged group."""
    dtype, bands = PELS[pel]
    lanes = lib.vips_hip_cells_step(2, pel) * lib.vips_hip_cells_step(0, pel)
    per_group = lib.vips_hip_cells_step(1, pel) // pel
    hspacing, shim, vspacing = 1028, 13 if pel == 4 else 12, 70
    width = 2 * hspacing + shim
    groups = -(-width // per_group)
    rows_of_cells = lanes // groups // (vspacing + shim) + 2
    height = rows_of_cells * (vspacing + shim) - shim
    assert width % per_group and width * pel % 4 == 0 and groups * height > lanes
    # the first step ends above the last row of cells
    assert lanes // groups < height - vspacing
    n = 2 * rows_of_cells - 1
    arrays = [noise(1024 if i % 3 else 1028, vspacing - 8 * (i % 2) - 3 * (i == n - 1), dtype, bands, 900 + i) for i in range(n)]
    kw = dict(across=2, shim=shim, halign="centre", valign="low", hspacing=hspacing, vspacing=vspacing, background=[10, 200, 30, 77][:bands])
    want, _ = model.ref_arrayjoin(tmp_path, [(a, INTERP["srgb"]) for a in arrays], model.cli_options(**kw))
    assert want.shape == (height, width, bands)
    got, _, ran = dev_arrayjoin(arrays, **kw)
    assert ran == {"cells_stream": 1}, ran
    same(got, want, ("second turn", pel))


@pytest.mark.parametrize("case", [(3, 1), (2, 3), (4, 1), (8, 3), (24, 1)], ids=lambda c: "pel%d-%dblocks" % c)
def test_cells_general_second_turn(case):
    """The one-pel-a-lane kernel with more rows than grid.y (the cap for a sheet one block wide, a third of it for three
    blocks), copying units of 1, 2, 4 and 8 bytes: cells' edges, shims and images' bottom edges in the second turn."""
    pel, blocks = case
    dtype, bands = PELS[pel]
    threads, cap = lib.vips_hip_cells_step(0, pel), lib.vips_hip_cells_step(2, pel)
    hspacing, shim = ((blocks - 1) * threads + 40) // 2, 1
    width = 2 * hspacing + shim
    in_flight = -(-cap // blocks)
    vspacing = in_flight // 3
    height = 4 * (vspacing + shim) - shim
    assert -(-width // threads) == blocks and width % 2 and height > in_flight + vspacing and (blocks == 1) == (in_flight == cap)
    arrays = [noise(hspacing - i % 3, vspacing - 5 * (i % 2), dtype, bands, 920 + i) for i in range(7)]
    kw = dict(across=2, shim=shim, halign="high", valign="centre", hspacing=hspacing, vspacing=vspacing, background=[10, 200, 30, 77][:bands])
    with general_kernel():
        got, _, ran = dev_arrayjoin(arrays, **kw)
    assert ran == {"cells_general": 1}, ran
    want = model_arrayjoin(arrays, **kw)
    assert want.shape == (height, width, bands)
    same(got, want, ("second turn", pel, blocks))


@pytest.mark.parametrize("blocks", [1, 3])
@pytest.mark.parametrize("nick", ["zoom", "subsample"])
def test_zoom_and_subsample_second_turn(nick, blocks):
    """Narrow and tall: more output rows than a launch has in flight -- the block budget over the blocks of a row,
    rounded down -- for rows of one block and of three (the last ragged)."""
    threads, cap = lib.vips_hip_upsize_step(0), lib.vips_hip_upsize_step(1)
    in_flight = cap // blocks
    xfac, yfac = 3, 2
    out_width, out_height = ((blocks - 1) * threads + 42) // xfac * xfac, (in_flight + 5) // yfac * yfac
    assert -(-out_width // threads) == blocks and out_width % threads and out_height > in_flight
    dtype, bands, interp = ((np.uint8, 3, "srgb"), (np.uint8, 1, "b-w"))[blocks // 2]
    if nick == "zoom":
        src = noise(out_width // xfac, out_height // yfac, dtype, bands, 940)
    else:
        src = noise(out_width * xfac + 1, out_height * yfac + 1, dtype, bands, 941)
    got = both(lambda: getattr(Image.new_from_array(src, interp), nick)(xfac, yfac),
               lambda: model.ref_input(nick, src, "xfac=%d,yfac=%d" % (xfac, yfac), INTERP[interp]), (nick, blocks), (nick,))
    assert (got.height, got.width) == (out_height, out_width)


# ---------------------------------------------------------------- 7. the region forms

def need_of(fn, *args):
    need = (ctypes.c_int * 4)()
    fn(*(args + (need,)))
    return tuple(need)


@pytest.mark.parametrize("kernel", ["stream", "general"])
def test_replicate_gen_strip_by_strip(kernel):
    """Strips of one row from the window of the input that vips_hip_replicate_need names: a row of the image while a
    strip stays inside a period across, the whole width once it crosses one; rows off dwords take the one-pel-a-lane
    kernel; a need withheld is refused."""
    src = noise(12, 7, np.uint8, 3, 900)
    x0, y0, size = 5, 3, (40, 20)
    whole = model.replicate(src, 0, 0, x0, y0, *size)
    for left, width in ((0, 40), (8, 6), (3, 20)):
        for top in range(0, 20, 3):
            need = need_of(lib.vips_hip_replicate_need, 12, 7, x0, y0, left, top, width, 1)
            assert need[3] == 1 and need[1] == (top + y0) % 7
            assert (need[0], need[2]) == (((left + x0) % 12, width) if (left + x0) % 12 + width <= 12 else (0, 12))
            for margin in (4, 1):
                with general_kernel(kernel == "general"), gated() as g:
                    got = gen_in_frames(lambda ri, ro: lib.vips_hip_replicate_gen(x0, y0, ri, ro), src, size, in_window=need,
                                        out_rect=(left, top, width, 1), margin=margin)
                assert g.ran == expect_kernel(kernel, 3, margin == 4), g.ran
                same(got, whole[top:top + 1, left:left + width], (kernel, left, width, top, margin))
    # a rect of several periods down needs every row; one row less is refused
    need = need_of(lib.vips_hip_replicate_need, 12, 7, x0, y0, 0, 2, 40, 9)
    assert need == (0, 0, 12, 7)
    same(gen_in_frames(lambda ri, ro: lib.vips_hip_replicate_gen(x0, y0, ri, ro), src, size, in_window=need, out_rect=(0, 2, 40, 9)),
         whole[2:11], "rows of two periods")
    lib.vips_hip_error_clear()
    with pytest.raises(VipsHipError, match="replicate: input region too small"):
        gen_in_frames(lambda ri, ro: lib.vips_hip_replicate_gen(x0, y0, ri, ro), src, size, in_window=(0, 1, 12, 6),
                      out_rect=(0, 2, 40, 9))
    with pytest.raises(VipsHipError, match="replicate: input region too small"):
        gen_in_frames(lambda ri, ro: lib.vips_hip_replicate_gen(x0, y0, ri, ro), src, size, in_window=(1, 0, 11, 7),
                      out_rect=(0, 2, 40, 1))


@pytest.mark.parametrize("kernel", ["stream", "general"])
def test_grid_gen_strip_by_strip(kernel):
    """One tile across: a strip of one row draws on one row.  Three across: on the rows from the first tile's to the
    last tile's, which is most of the strip; a row of that need withheld is refused."""
    src = noise(8, 60, np.uint16, 2, 910)
    for tile_height, across, down in ((20, 1, 3), (5, 3, 4), (1, 4, 15)):
        size = (8 * across, tile_height * down)
        whole = model.grid(src, tile_height, across, down)
        for top in range(0, size[1], max(1, size[1] // 7)):
            need = need_of(lib.vips_hip_grid_need, 8, 60, tile_height, across, 0, top, size[0], 1)
            ty, ry = divmod(top, tile_height)
            first = ty * across * tile_height + ry
            assert need == (0, first, 8, (across - 1) * tile_height + 1), (need, tile_height, across, top)
            for margin in (4, 1):
                with general_kernel(kernel == "general"), gated() as g:
                    got = gen_in_frames(lambda ri, ro: lib.vips_hip_grid_gen(tile_height, across, ri, ro), src, size,
                                        in_window=need, out_rect=(0, top, size[0], 1), margin=margin)
                assert g.ran == expect_kernel(kernel, 4), g.ran  # (a 4-byte pel: rows start on dwords with any margin)
                same(got, whole[top:top + 1], (kernel, tile_height, across, top, margin))
            # a rect inside one tile: that tile's rows and columns alone
            tx = across - 1
            need = need_of(lib.vips_hip_grid_need, 8, 60, tile_height, across, 8 * tx + 2, top, 5, 1)
            assert need == (2, (ty * across + tx) * tile_height + ry, 5, 1)
            got = gen_in_frames(lambda ri, ro: lib.vips_hip_grid_gen(tile_height, across, ri, ro), src, size, in_window=need,
                                out_rect=(8 * tx + 2, top, 5, 1))
            same(got, whole[top:top + 1, 8 * tx + 2:8 * tx + 7], ("one tile", tile_height, across, top))
        if across > 1:
            need = need_of(lib.vips_hip_grid_need, 8, 60, tile_height, across, 0, 0, size[0], 1)
            lib.vips_hip_error_clear()
            with pytest.raises(VipsHipError, match="grid: input region too small"):
                gen_in_frames(lambda ri, ro: lib.vips_hip_grid_gen(tile_height, across, ri, ro), src, size,
                              in_window=(0, 0, 8, need[3] - 1), out_rect=(0, 0, size[0], 1))


# ---------------------------------------------------------------- 8. refusals by name

def test_refusals():
    lib.vips_hip_error_clear()
    cx = Image.new_from_array(np.ones((4, 4, 2), np.complex64))
    wide = Image.new_from_array(noise(4, 4, np.float64, 5, 950))
    ok = Image.new_from_array(noise(4, 4, np.uint8, 3, 951))
    for name, call in (("arrayjoin", lambda im: Image.arrayjoin([im, im])), ("replicate", lambda im: im.replicate(2, 2)),
                       ("wrap", lambda im: im.wrap()), ("grid", lambda im: im.grid(2, 1, 2))):
        with pytest.raises(VipsHipError, match=name + ": image must be non-complex"):
            call(cx)
        with pytest.raises(VipsHipError, match=name + ": pels of more than 32 bytes are outside the HIP path"):
            call(wide)
    for name, call in (("zoom", lambda im: im.zoom(2, 2)), ("subsample", lambda im: im.subsample(2, 2))):
        with pytest.raises(VipsHipError, match=name + ": image must be non-complex"):
            call(cx)
    with pytest.raises(VipsHipError, match="arrayjoin: no input images"):
        Image.arrayjoin([])
    with pytest.raises(VipsHipError, match="grid: bad grid geometry"):
        ok.grid(3, 1, 1)
    with pytest.raises(VipsHipError, match="replicate: output size overflows an int"):
        Image.new_from_array(noise(4096, 1, np.uint8, 1, 952)).replicate(1000000, 1)
    with pytest.raises(VipsHipError, match="enum 'VipsAlign' has no member"):
        Image.arrayjoin([ok], halign=7)


def test_images_on_different_devices_are_refused():
    if lib.vips_hip_device_count() < 2:
        pytest.skip("one GPU")
    a = Image.new_from_array(noise(4, 4, np.uint8, 3, 960))
    libvips_amd.init(1)
    try:
        b = Image.new_from_array(noise(4, 4, np.uint8, 3, 961))
    finally:
        libvips_amd.init(0)
    lib.vips_hip_error_clear()
    with pytest.raises(VipsHipError, match="arrayjoin: the images are on different devices"):
        Image.arrayjoin([a, b])


# ---------------------------------------------------------------- 9. the libvips module

# (on host fibers the library under test is not the one the module was linked against)
needs_module = pytest.mark.skipif(not helpers.have_module() or bool(os.environ.get("VIPS_HIP_LIBRARY")),
                                  reason="host/_build missing, or another build of the library is under test")


@needs_module
@pytest.mark.parametrize("strips", [False, True], ids=["whole", "strips"])
def test_module_cells_classes(strips):
    """replicate_hip, wrap_hip, grid_hip, zoom_hip and subsample_hip make the built-in operations' pixels, whole and
    strip by strip (a small $VIPS_HIP_BUDGET, as tests/test_module.py)."""
    Ref.load_module()
    module = ctypes.CDLL(helpers.MODULE_LIB)
    height = 720 if strips else 60
    src = helpers.lcg_image(400, height, 4, np.uint8, 970)
    cases = [("replicate", "across=2,down=3"), ("replicate", "across=1,down=1"), ("wrap", ""), ("wrap", "x=-37,y=%d" % (height + 11)),
             ("wrap", "x=400,y=0"), ("grid", "tile_height=%d,across=1,down=3" % (height // 3)),
             ("grid", "tile_height=%d,across=3,down=4" % (height // 12)), ("grid", "tile_height=1,across=4,down=%d" % (height // 4)),
             ("zoom", "xfac=2,yfac=3"), ("subsample", "xfac=3,yfac=2"), ("subsample", "xfac=11,yfac=1,point=true")]
    if strips:
        os.environ["VIPS_HIP_BUDGET"] = "300k"
    before = module.vips_hip_module_strips_done()
    try:
        for nick, args in cases:
            # (the module's classes all name their image "in"; vips_zoom and vips_subsample name theirs "input")
            original = model.ref_input if nick in ("zoom", "subsample") else Ref.run_interp
            got, got_interp = Ref.run_interp(nick + "_hip", src, args, interpretation=INTERP["srgb"])
            want, want_interp = original(nick, src, args, interpretation=INTERP["srgb"])
            same(got, want, "%s_hip %s" % (nick, args))
            assert got_interp == want_interp
    finally:
        if strips:
            del os.environ["VIPS_HIP_BUDGET"]
    if strips:
        assert module.vips_hip_module_strips_done() - before >= 2 * len(cases), "not strip-mined"


@needs_module
def test_module_errors():
    Ref.load_module()
    src = noise(40, 30, np.uint8, 3, 980)
    with pytest.raises(RuntimeError, match="grid_hip: bad grid geometry"):
        Ref.run("grid_hip", src, "tile_height=7,across=2,down=2")
    with pytest.raises(RuntimeError, match="subsample_hip: image has shrunk to nothing"):
        Ref.run("subsample_hip", src, "xfac=41,yfac=1")
    with pytest.raises(RuntimeError, match="zoom_hip: zoom factors too large"):
        Ref.run("zoom_hip", noise(120, 4, np.uint8, 3, 981), "xfac=10000000,yfac=1")
