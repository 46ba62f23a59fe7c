"""GPU parity: vips_affine / vips_similarity / vips_rotate (libvips_amd/csrc/affine.hip, interp_device.h, ops_affine.cpp).

The reference is deterministic whatever its thread count (a pixel's coordinates depend on its 128 x 128 sink tile and
on nothing else), and the device repeats its arithmetic operation by operation, so every comparison is np.array_equal
against the compiled reference, shapes and dtypes included.  Every case asserts which kernel ran, by the gate report.

The cases are a sparse cross: every matrix x every interpolator on uchar with 1, 3 and 4 bands; three matrices x every
interpolator on the other formats; the arguments, the extend modes and the alpha chain on their own.  Output sizes sit
round the 128-column rect grid (127, 128, 129, 261).  The grid case (test_the_rect_grid_shows) is the one an
implementation that walks whole rows, or multiplies instead of accumulating, fails: it carries a numpy restatement of
the walk and first proves on the CPU that the restart is visible on its input.
Float inputs are positive noise: no NaN, no -0.  Runs on the CPU too, on host fibers (tests/test_emul_affine.py)."""
import ctypes
import math
import os

import numpy as np
import pytest

import libvips_amd
from libvips_amd import Image, VipsHipError, _ffi
from tests import helpers
from tests.helpers import Ref

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not helpers.have_ref(), reason="oracle/_ref not built")]

lib = _ffi.lib
INTERPOLATORS = ("nearest", "bilinear", "bicubic")
SIZES = (127, 128, 129, 261)
SRGB, B_W = 22, 1


@pytest.fixture(scope="module", autouse=True)
def _init():
    libvips_amd.init(0)


class gated(object):
    """with gated() as g: ...; g.ran: {gate name: launches} of the affine kernels that ran inside."""

    def __enter__(self):
        lib.vips_hip_gate_reset()
        lib.vips_hip_gate_enable(1)
        self.ran = None
        return self

    def __exit__(self, *exc):
        try:
            if exc[0] is None:
                self.ran = {k: n for k, (n, _) in libvips_amd.gate_report().items() if k.startswith("affine_")}
        finally:
            lib.vips_hip_gate_enable(0)
            lib.vips_hip_gate_reset()
        return False


_noise = {}


def noise(w, h, bands, dtype=np.uint8, seed=11):
    """A w x h corner of one noise image per (bands, dtype, seed): made once, never changed."""
    key = (bands, np.dtype(dtype), seed)
    if key not in _noise or _noise[key].shape[0] < h or _noise[key].shape[1] < w:
        _noise[key] = helpers.lcg_image(max(w, 400), max(h, 400), bands, dtype, seed)
    a = np.ascontiguousarray(_noise[key][:h, :w])
    if np.dtype(dtype).kind == "f":
        a = a + np.float32(1)  # strictly positive
        assert not np.isnan(a).any() and (a > 0).all()
    return a


def same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d of %d differ, first at %s: got %r want %r" % (
            what, len(bad), got.size, bad[0], got[tuple(bad[0])], want[tuple(bad[0])]))


def vec(values):
    return " ".join(repr(float(v)) for v in values)


def ref_args(kw):
    """The reference's argument string of pyvips-style keyword arguments."""
    parts = []
    for key, value in kw.items():
        if key in ("matrix", "background"):
            parts.append("%s=%s" % (key, vec(np.atleast_1d(value))))
        elif key == "oarea":
            parts.append("oarea=" + " ".join(str(int(v)) for v in value))
        elif key == "premultiplied":
            parts.append("premultiplied=%s" % ("true" if value else "false"))
        elif key in ("interpolate", "extend"):
            parts.append("%s=%s" % (key, value))
        else:
            parts.append("%s=%r" % (key, float(value)))
    return ",".join(parts)


def check(op, src, expect_gate=True, interpretation=0, **kw):
    """One operation on the device against the reference; the gate of its interpolator ran once and no other."""
    want = Ref.run(op, src, ref_args(kw), interpretation=interpretation)
    im = Image.new_from_array(src, interpretation=interpretation)
    py = dict(kw)
    with gated() as g:
        if op == "affine":
            got = im.affine(py.pop("matrix"), **py).numpy()
        elif op == "similarity":
            got = im.similarity(py.pop("scale", 1.0), py.pop("angle", 0.0), **py).numpy()
        else:
            got = im.rotate(py.pop("angle"), **py).numpy()
    what = "%s %s on %s %s" % (op, ref_args(kw), src.shape, src.dtype)
    gate = {"affine_" + kw.get("interpolate", "bilinear"): 1} if expect_gate else {}
    assert g.ran == gate, (what, g.ran)
    same(got, want, what)
    return got


# ---- matrices x interpolators x formats

def oarea_of(k, left=-20, top=-30):
    return (left, top, SIZES[k % 4], SIZES[(k + 1) % 4])


MATRICES = {
    "rotate7": ("rotate", dict(angle=7)),
    "rotate30": ("rotate", dict(angle=30)),
    "rotate33.3": ("rotate", dict(angle=33.3)),
    "rotate90": ("rotate", dict(angle=90)),
    "rotate180": ("rotate", dict(angle=180)),
    "rotate-100": ("rotate", dict(angle=-100)),
    "similarity0.37": ("similarity", dict(scale=0.37, angle=12.5)),
    "similarity2.5": ("similarity", dict(scale=2.5, angle=-100)),
    "shear": ("affine", dict(matrix=(1.3, 0.2, 0.1, 0.9), oarea=oarea_of(0))),
    # (an area that ends left of the origin is "out of range" in the reference: this one crosses it)
    "reflection": ("affine", dict(matrix=(-1, 0, 0, 1), oarea=(-150, -10, SIZES[3], SIZES[2]))),
    "scale_down": ("affine", dict(matrix=(0.4, 0, 0, 0.4))),
    "scale_up": ("affine", dict(matrix=(2.5, 0, 0, 1.5), oarea=(-3, -2, SIZES[3], SIZES[0]))),
    "identity": ("affine", dict(matrix=(1, 0, 0, 1))),
    "identity_oarea": ("affine", dict(matrix=(1, 0, 0, 1), oarea=oarea_of(2, -5, -7))),
}


@pytest.mark.parametrize("name", sorted(MATRICES))
def test_matrices_uchar(name):
    """Every matrix x every interpolator x 1, 3 and 4 bands on uchar (no alpha: the interpretation is multiband).
    rotate 90 and 180 are general transforms (cos(pi / 2) is not 0 in doubles); the pure scales take the whole-row
    route; the identity with the image's own area is the copy and launches nothing."""
    op, kw = MATRICES[name]
    for bands in (1, 3, 4):
        src = noise(150, 100, bands, np.uint8, 11 + bands)
        for interpolate in INTERPOLATORS:
            check(op, src, expect_gate=name != "identity", interpolate=interpolate, **kw)


@pytest.mark.parametrize("dtype", [np.uint16, np.int16, np.int32, np.float32, np.int8, np.uint32],
                         ids=lambda d: np.dtype(d).name)
def test_formats(dtype):
    """The formats beside uchar on a rotation, the shear and the enlargement, every interpolator, 1 and 3 bands.
    Integer noise is full range, so signed formats cross zero and the bicubic's clip works at both ends."""
    for bands in (1, 3):
        src = noise(140, 90, bands, dtype, 31 + bands)
        for interpolate in INTERPOLATORS:
            for name in ("rotate33.3", "shear", "scale_up"):
                op, kw = MATRICES[name]
                check(op, src, interpolate=interpolate, **kw)


def test_moved_pixels_show():
    """An index image (every pel its own value): nearest through a quarter turn and the reflection are permutations."""
    src = (np.arange(90 * 70, dtype=np.uint16).reshape(70, 90, 1) + 1).astype(np.uint16)
    got = check("rotate", src, angle=90, interpolate="nearest")
    assert len(np.unique(got)) > 90 * 60
    check("affine", src, matrix=(-1, 0, 0, 1), interpolate="nearest")
    check("affine", src, matrix=(0, 1, -1, 0), interpolate="nearest")


# ---- the arguments

@pytest.mark.parametrize("interpolate", INTERPOLATORS)
def test_oarea(interpolate):
    """Negative origin, partly outside the image, and wholly outside it (every rect is background)."""
    src = noise(150, 100, 3, np.uint8, 41)
    m = (0.8, 0.6, -0.6, 0.8)
    for oarea in ((-10, -20, 333, 150), (100, 60, 129, 127), (-60, 120, 128, 261), (1000, 1000, 129, 127)):
        check("affine", src, matrix=m, oarea=oarea, interpolate=interpolate, background=(10, 20, 30))


@pytest.mark.parametrize("interpolate", INTERPOLATORS)
def test_displacements(interpolate):
    src = noise(150, 100, 3, np.uint8, 43)
    check("affine", src, matrix=(1.3, 0.2, 0.1, 0.9), oarea=(-10, -20, 261, 129), odx=1.5, idy=-2.25,
          background=(10, 20, 30), extend="background", interpolate=interpolate)
    check("affine", src, matrix=(1.3, 0.2, 0.1, 0.9), ody=-7.75, idx=3.3, interpolate=interpolate)
    check("affine", src, matrix=(2.5, 0, 0, 1.5), odx=0.25, ody=11.5, idx=-1.75, idy=0.5, interpolate=interpolate)
    check("similarity", src, scale=0.37, angle=12.5, odx=1.5, ody=2.5, idx=-3.25, idy=4.125, interpolate=interpolate)
    check("rotate", src, angle=33.3, odx=-1.5, idy=7.2, interpolate=interpolate)


def test_background_lengths():
    for bands, dtype in ((3, np.uint8), (1, np.uint8), (3, np.int16), (3, np.float32)):
        src = noise(100, 60, bands, dtype, 45)
        check("rotate", src, angle=30, background=77.7)
        check("rotate", src, angle=30, background=[1.5, -300, 70000.25][:bands])
        check("affine", src, matrix=(0.8, 0.6, -0.6, 0.8), background=[12, 250, 99][:bands], extend="black")


@pytest.mark.parametrize("extend", ["black", "copy", "repeat", "mirror", "white", "background"])
def test_extend_modes(extend):
    """Every way the edge is continued, on an image smaller than the stencil and on one of a tile + 1; the output
    area reaches past the image on every side so the pels the embed invents are read."""
    for (w, h) in ((3, 2), (129, 129)):
        for dtype in (np.uint8, np.int16):
            src = noise(w, h, 3, dtype, 47)
            for interpolate in INTERPOLATORS:
                check("affine", src, matrix=(1.5, 0.3, -0.2, 1.4), oarea=(-12, -9, int(1.8 * w) + 24, int(1.6 * h) + 20),
                      extend=extend, background=(40, 50, 60), interpolate=interpolate)
                check("affine", src, matrix=(2.5, 0, 0, 1.5), oarea=(-7, -5, int(2.5 * w) + 14, int(1.5 * h) + 10),
                      extend=extend, background=(40, 50, 60), interpolate=interpolate)


# ---- alpha

@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float32], ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("bands", [2, 4])
def test_alpha(dtype, bands):
    """Images with alpha (by interpretation: b-w with 2 bands, srgb with 4) go through premultiply -> affine ->
    unpremultiply -> cast unless premultiplied is set; the fill round the image is premultiplied, the ink is not."""
    interpretation = B_W if bands == 2 else SRGB
    src = noise(140, 90, bands, dtype, 51 + bands)
    for premultiplied in (False, True):
        for extend in ("background", "white"):
            for interpolate in INTERPOLATORS:
                check("affine", src, interpretation=interpretation, matrix=(0.8, 0.6, -0.6, 0.8),
                      oarea=(-30, -40, 261, 129), premultiplied=premultiplied, extend=extend,
                      background=[200, 100, 50, 128][4 - bands:], interpolate=interpolate)
    check("rotate", src, interpretation=interpretation, angle=33.3, background=[200, 100, 50, 128][4 - bands:])


# ---- the grid case

def walk_model(src, ia, ib, ic, id_, oarea, interpolate, tile):
    """The reference's generate restated (affine.c:324-403) for a one-band uchar or ushort image, extend background 0, no
    displacements: the inverse matrix applied to a rect's first pixel of each row, then `+= ddx`, floor, clip, and the
    nearest / 12-bit bilinear fetch through the embed.  `tile`: where rects start (0: whole rows)."""
    H, W = src.shape[:2]
    left, top, ow, oh = oarea
    wo = 0
    ws = 1 if interpolate == "nearest" else 2
    emb = np.zeros((H + ws - 1 + 2, W + ws - 1 + 2), np.int64)
    emb[wo + 1:wo + 1 + H, wo + 1:wo + 1 + W] = src[:, :, 0]
    oy = (np.arange(oh, dtype=np.int64) + top).astype(np.float64) - 0.0
    xs = np.empty((oh, ow), np.float64)
    ys = np.empty((oh, ow), np.float64)
    step = tile if tile else ow
    for le in range(0, ow, step):
        ox = np.float64(le + left) - 0.0
        x = ia * ox + ib * oy
        y = ic * ox + id_ * oy
        x = x - (-1.0)
        y = y - (-1.0)
        x = x + np.float64(wo)
        y = y + np.float64(wo)
        for col in range(le, min(le + step, ow)):
            xs[:, col] = x
            ys[:, col] = y
            x = x + ia
            y = y + ic
    fx = np.floor(xs)
    fy = np.floor(ys)
    inside = (fx >= wo) & (fx <= wo + W) & (fy >= wo) & (fy <= wo + H)
    ix = np.where(inside, xs, 0).astype(np.int64)
    iy = np.where(inside, ys, 0).astype(np.int64)
    if interpolate == "nearest":
        v = emb[iy, ix]
    else:
        X = ((np.where(inside, xs, 0) - ix) * 4096).astype(np.int64)
        Y = ((np.where(inside, ys, 0) - iy) * 4096).astype(np.int64)
        Yd = 4096 - Y
        c4 = (Y * X) >> 12
        c2 = (Yd * X) >> 12
        c3 = Y - c4
        c1 = Yd - c2
        v = (c1 * emb[iy, ix] + c2 * emb[iy, ix + 1] + c3 * emb[iy + 1, ix] + c4 * emb[iy + 1, ix + 1] + 2048) >> 12
    out = np.where(inside, v, 0).astype(src.dtype)
    return out[:, :, None], (fx, fy)


def inverse(a, b, c, d):
    tmp = 1.0 / (a * d - b * c)
    return tmp * d, -tmp * b, -tmp * c, tmp * a


GRID_CASES = {
    # rotate 45 of 362 x 362 is 512 x 512: four columns of sink tiles
    "rotate45": ("rotate", dict(angle=45), None),
    "rotate30x2.5": ("affine", dict(matrix=(2.165063509461097, -1.25, 1.25, 2.165063509461097)), (-452, 0, 1024, 640)),
}
_grid_ref = {}


@pytest.mark.parametrize("interpolate", ["nearest", "bilinear"])
@pytest.mark.parametrize("name", sorted(GRID_CASES))
def test_the_rect_grid_shows(name, interpolate):
    """The case that fails for a walk along whole rows or for start + k * ddx.  First, on the CPU: the restated walk
    with the 128-column restart IS the reference on every pixel, and the same walk along whole rows is NOT (so the
    input can tell the two apart); then the device equals the reference."""
    op, kw, oarea = GRID_CASES[name]
    # ushort for bilinear: a 12-bit weight that is one off moves a uchar result a few times in a hundred, a ushort
    # result nearly always (on uchar noise the 30 degree case hides all of its 31 pixels)
    src = noise(362, 362, 1, np.uint8 if interpolate == "nearest" else np.uint16, 61)
    if op == "rotate":
        rad = (kw["angle"] / 360.0) * 2.0 * math.pi
        a = 1.0 * math.cos(rad)
        b = 1.0 * -math.sin(rad)
        m = (a, b, -b, a)
    else:
        m = kw["matrix"]
    kw = dict(kw, interpolate=interpolate)
    if oarea is not None:
        kw["oarea"] = oarea
    want = Ref.run(op, src, ref_args(kw))
    if oarea is None:
        # vips__transform_set_area: the rounded bounding box of the forward-mapped corners
        xs = [m[0] * x + m[1] * y for x in (0, 362) for y in (0, 362)]
        ys = [m[2] * x + m[3] * y for x in (0, 362) for y in (0, 362)]
        rnd = lambda r: int(r + 0.5) if r > 0 else int(r - 0.5)
        oarea = (rnd(min(xs)), rnd(min(ys)), rnd(max(xs) - min(xs)), rnd(max(ys) - min(ys)))
    assert want.shape[1] >= 512 and want.shape[:2] == (oarea[3], oarea[2])
    inv = inverse(*m)
    tiled, _ = walk_model(src, *inv, oarea, interpolate, 128)
    same(tiled, want, "the restated walk with the 128 restart, %s %s" % (name, interpolate))
    rows, _ = walk_model(src, *inv, oarea, interpolate, 0)
    differ = int((rows != want).sum())
    print("%s %s: a whole-row walk differs from the reference on %d of %d pixels" % (name, interpolate, differ, want.size))
    assert differ >= 1, "this input cannot tell the rect grid from whole rows: choose another"
    check(op, src, **kw)


# ---- regions

def plan_of(src, interpretation=0, **kw):
    args = Image.affine_args(**kw)
    h, w, b = src.shape
    plan = lib.vips_hip_affine_plan_new(ctypes.byref(args), w, h, b, libvips_amd.image.DTYPE_FORMATS[src.dtype], interpretation)
    return _ffi.check_handle(plan)


def need_of(plan, rect):
    out = (ctypes.c_int * 4)()
    lib.vips_hip_affine_need(plan, rect[0], rect[1], rect[2], rect[3], out)
    return tuple(out)


def region_pair(src, window, rect, out_size):
    """The window (left, top, w, h) of src as an input region, and an output region for rect of an image out_size."""
    x0, y0, w, h = window
    H, W = src.shape[:2]
    win = Image.new_from_array(np.ascontiguousarray(src[y0:y0 + h, x0:x0 + w]))
    rin = win.region()
    rin.left, rin.top, rin.im_width, rin.im_height = x0, y0, W, H
    out = Image.new_from_array(np.zeros((rect[3], rect[2], src.shape[2]), src.dtype))
    rout = out.region()
    rout.left, rout.top, rout.im_width, rout.im_height = rect[0], rect[1], out_size[0], out_size[1]
    return win, rin, out, rout


@pytest.mark.parametrize("interpolate", INTERPOLATORS)
@pytest.mark.parametrize("case", ["rotate", "scale", "mirror"])
def test_region_form(case, interpolate):
    """vips_hip_affine_gen on rects that start off the grid origin and on a strip, from an input window that is
    exactly vips_hip_affine_need of the rect: the same rect of the whole-image result.  A window one row short is
    refused and nothing is launched."""
    src = noise(200, 150, 3, np.uint8, 71)
    if case == "rotate":
        kw = dict(matrix=(0.8, 0.6, -0.6, 0.8), interpolate=interpolate, background=(9, 8, 7))
    elif case == "scale":
        kw = dict(matrix=(1.7, 0, 0, 2.2), interpolate=interpolate, idx=0.4)
    else:  # (a rect that touches the embed's border reads the far side of the image)
        kw = dict(matrix=(1.3, 0.2, 0.1, 0.9), interpolate=interpolate, extend="mirror", oarea=(-15, -12, 300, 190))
    whole = check("affine", src, **kw)
    oh, ow = whole.shape[:2]
    plan = plan_of(src, **kw)
    try:
        assert (lib.vips_hip_affine_plan_get(plan, 0), lib.vips_hip_affine_plan_get(plan, 1)) == (ow, oh)
        tile = lib.vips_hip_affine_plan_get(plan, 3)
        assert tile == (0 if case == "scale" else 128)
        for rect in ((37, 21, 150, 60), (130, 3, 41, 140), (0, 64, ow, 32), (ow - 9, oh - 7, 9, 7), (0, 0, 5, 5)):
            need = need_of(plan, rect)
            if need[2] == 0:
                need = (0, 0, 1, 1)  # all background: any window
            win, rin, out, rout = region_pair(src, need, rect, (ow, oh))
            with gated() as g:
                _ffi.check(lib.vips_hip_affine_gen(plan, ctypes.byref(rin), ctypes.byref(rout), tile))
                got = out.numpy()
            assert g.ran == {"affine_" + interpolate: 1}
            same(got, np.ascontiguousarray(whole[rect[1]:rect[1] + rect[3], rect[0]:rect[0] + rect[2]]), "region %r" % (rect,))
        rect = (37, 21, 150, 60)
        need = need_of(plan, rect)
        assert need[3] > 2
        win, rin, out, rout = region_pair(src, (need[0], need[1], need[2], need[3] - 1), rect, (ow, oh))
        lib.vips_hip_error_clear()
        with gated() as g:
            assert lib.vips_hip_affine_gen(plan, ctypes.byref(rin), ctypes.byref(rout), tile) == -1
        assert "affine: input region too small" in _ffi.error_buffer()
        assert g.ran == {}
        lib.vips_hip_error_clear()
    finally:
        lib.vips_hip_affine_plan_free(plan)


# ---- errors and refusals

def test_errors_and_refusals():
    src = noise(60, 40, 3, np.uint8, 81)
    im = Image.new_from_array(src)
    with pytest.raises(VipsHipError, match="singular or near-singular matrix"):
        im.affine((1, 2, 2, 4))
    with pytest.raises(RuntimeError, match="singular or near-singular matrix"):
        Ref.run("affine", src, "matrix=1 2 2 4")
    with pytest.raises(VipsHipError, match="affine: output coordinates out of range"):
        im.affine((0.8, 0.6, -0.6, 0.8), oarea=(0, 0, 2 ** 30, 10))
    with pytest.raises(RuntimeError, match="output coordinates out of range"):
        Ref.run("affine", src, "matrix=0.8 0.6 -0.6 0.8,oarea=0 0 %d 10" % 2 ** 30)
    # (the reference's test is unsigned: an area that ends left of the origin is out of range as well)
    with pytest.raises(VipsHipError, match="affine: output coordinates out of range"):
        im.affine((0.8, 0.6, -0.6, 0.8), oarea=(-400, 0, 333, 10))
    with pytest.raises(RuntimeError, match="output coordinates out of range"):
        Ref.run("affine", src, "matrix=0.8 0.6 -0.6 0.8,oarea=-400 0 333 10")
    with pytest.raises(VipsHipError, match="linear: vector must have 1 or 3 elements"):
        im.rotate(30, background=[1, 2])
    with pytest.raises(RuntimeError, match="linear: vector must have 1 or 3 elements"):
        Ref.run("rotate", src, "angle=30,background=1 2")
    # what the device does not take is refused by name: no other path runs it
    with gated() as g:
        with pytest.raises(VipsHipError, match="affine: double images"):
            Image.new_from_array(noise(60, 40, 1, np.float64, 82)).rotate(30)
        with pytest.raises(VipsHipError, match="affine: complex images"):
            Image.new_from_array(noise(60, 40, 1, np.float32, 82).astype(np.complex64)).rotate(30)
        for name in ("nohalo", "lbb", "vsqbs"):
            with pytest.raises(VipsHipError, match="affine: interpolator %s is outside the HIP path" % name):
                im.rotate(30, interpolate=name)
    assert g.ran == {}


# ---- the libvips module

# (on host fibers the library under test is not the one the module was linked against)
needs_module = pytest.mark.skipif(not helpers.have_module() or bool(os.environ.get("VIPS_HIP_LIBRARY")),
                                  reason="host/_build missing, or another build of the library is under test")


@needs_module
@pytest.mark.parametrize("strips", [False, True], ids=["whole", "strips"])
def test_module_rotate_and_affine(strips):
    """rotate_hip, affine_hip and similarity_hip make the built-in operations' pixels, whole and strip by strip (a
    small $VIPS_HIP_BUDGET, as tests/test_module.py); what the device refuses is the original's."""
    Ref.load_module()
    module = ctypes.CDLL(helpers.MODULE_LIB)
    height = 700 if strips else 90
    src = helpers.lcg_image(300, height, 3, np.uint8, 91)
    rgba = helpers.lcg_image(120, height, 4, np.uint8, 92)
    if strips:
        os.environ["VIPS_HIP_BUDGET"] = "300k"
    before = module.vips_hip_module_strips_done()
    try:
        for op, args in (("rotate", "angle=33.3"),
                         ("affine", "matrix=1.3 0.2 0.1 0.9,interpolate=bicubic,oarea=-10 -20 333 %d,odx=1.5,idy=-2.25,"
                                    "background=10 20 30,extend=mirror" % (height + 30)),
                         ("affine", "matrix=2.5 0 0 1.5,interpolate=nearest"),
                         ("similarity", "scale=0.37,angle=12.5,interpolate=bicubic")):
            same(Ref.run(op + "_hip", src, args), Ref.run(op, src, args), "%s_hip %s" % (op, args))
        same(Ref.run("affine_hip", rgba, "matrix=0.8 0.6 -0.6 0.8,background=200 100 50 128", interpretation=SRGB),
             Ref.run("affine", rgba, "matrix=0.8 0.6 -0.6 0.8,background=200 100 50 128", interpretation=SRGB), "affine_hip rgba")
        # refused by the device path, so the original's
        same(Ref.run("rotate_hip", src[:60], "angle=30,interpolate=nohalo"), Ref.run("rotate", src[:60], "angle=30,interpolate=nohalo"),
             "rotate_hip nohalo")
        double = helpers.lcg_image(50, 40, 1, np.float64, 93)
        same(Ref.run("rotate_hip", double, "angle=30"), Ref.run("rotate", double, "angle=30"), "rotate_hip double")
    finally:
        if strips:
            del os.environ["VIPS_HIP_BUDGET"]
    if strips:
        assert module.vips_hip_module_strips_done() - before >= 5 * 2, "not strip-mined"


@needs_module
def test_module_build_moves_no_pixels_and_errors_are_the_originals():
    Ref.load_module()
    lib.vips_hip_pool_trim()
    before = lib.vips_hip_pool_bytes()
    for op, args in (("rotate", "angle=30"), ("affine", "matrix=1.3 0.2 0.1 0.9,oarea=-10 -20 3333 1500"),
                     ("similarity", "scale=0.37,angle=12.5")):
        got, secs = Ref.build_probe(op + "_hip", 20000, 20000, 3, args)
        want, _ = Ref.build_probe(op, 20000, 20000, 3, args)
        assert got == want and secs < 0.5, (op, got, want, secs)
    assert lib.vips_hip_pool_bytes() == before
    src = noise(60, 40, 3, np.uint8, 81)
    with pytest.raises(RuntimeError, match="singular or near-singular matrix"):
        Ref.run("affine_hip", src, "matrix=1 2 2 4")
    with pytest.raises(RuntimeError, match="affine_hip: output coordinates out of range"):
        Ref.run("affine_hip", src, "matrix=0.8 0.6 -0.6 0.8,oarea=0 0 %d 10" % 2 ** 30)
    with pytest.raises(RuntimeError, match="vector must have 1 or 3 elements"):
        Ref.run("rotate_hip", src, "angle=30,background=1 2")
