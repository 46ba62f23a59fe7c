"""GPU parity: vips_sobel / vips_scharr / vips_prewitt, vips_compass and vips_canny (libvips_amd/csrc/edge.hip,
ops_edge.cpp).

Every result is exact -- integer convolutions with their clips, or float operations rounded where the reference rounds
them -- so every comparison is np.array_equal against the compiled reference, shapes and dtypes included.  Every case
asserts which kernel family ran, by the gate report: uchar images take the fused kernel (edge_u8: one launch, no
convolution beside it), everything else two convolutions and the combine (edge_combine_f32).

Sizes: the ones where every pel is an edge pel (1 x 1, 1 x 7, 7 x 1, 2 x 2, 3 x 3), and one under / at / over a tile
and two tiles + 5 on both axes (vips_hip_edge_step: T_w elements x T_h rows), for 1, 3 and 4 bands; odd widths of 1-
and 3-band uchar images give rows whose stride is no multiple of 4.  Inputs: LCG noise (drives both clips of the
integer convolutions and the saturation behind them), a 0 / 255 step, horizontal, vertical and diagonal ramps, a white
disc on black, a constant image.

compass: uchar with precision integer and a 3 x 3 mask takes compass_u8 (one launch, no convolution), everything else
a convolution a distinct mask and compass_combine.  canny: a uchar blur takes canny_polar_thin_u8, any other
canny_polar_thin_f32; the float kernel's theta is the one spot that is not exact by construction, so every equality
stands beside `canny_marginal() == 0` (include/vips_hip.h: bit-identical whenever that counter is zero).
Runs on the CPU too, on host fibers (tests/test_emul_edge.py)."""
import ctypes

import numpy as np
import pytest

import libvips_amd
from libvips_amd import Image, VipsHipError, _ffi
from tests import helpers
from tests.helpers import Ref

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not helpers.have_ref(), reason="oracle/_ref not built")]

lib = _ffi.lib
BANDS = [1, 3, 4]
EDGES = ["sobel", "scharr", "prewitt"]
TINY = [(1, 1), (7, 1), (1, 7), (2, 2), (3, 3)]  # (width, height)


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


def tile():
    t = tuple(lib.vips_hip_edge_step(i) for i in range(2))
    assert all(v > 0 for v in t), t
    return t


def round_the_tile(bands):
    """Widths (pels) one under / at / over a tile's elements and two tiles + 5; heights the same for its rows."""
    tw, th = tile()
    at = -(-tw // bands)
    return (at - 1, at, at + 1, 2 * at + 5), (th - 1, th, th + 1, 2 * th + 5)


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


def patterns(w, h, bands):
    """The structured uchar inputs: name -> image.  Bands differ (band b is the pattern shifted by b pels)."""
    y, x = np.mgrid[0:h, 0:w + bands]
    base = {
        "step": np.where(x + y // 3 >= (w + bands) // 2, 255, 0),
        "hramp": (x * 3) % 256,
        "vramp": (y * 5) % 256,
        "dramp": (x + y) % 256,
        "disc": np.where((x - w / 2.0) ** 2 + (y - h / 2.0) ** 2 <= (min(w, h) / 3.0) ** 2, 255, 0),
        "constant": np.full_like(x, 77),
    }
    return {k: np.ascontiguousarray(np.stack([v[:, b:b + w] for b in range(bands)], axis=2).astype(np.uint8))
            for k, v in base.items()}


def same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d of %d differ, first at %s: got %r want %r" % (
            what, len(bad), got.size, bad[0], got[tuple(bad[0])], want[tuple(bad[0])]))


def families(report):
    """(launches by edge_* gate, launches of the convolution kernels)."""
    ran = {k: n for k, (n, _) in report.items() if k.startswith("edge_")}
    convs = sum(n for k, (n, _) in report.items() if k.startswith("conv"))
    return ran, convs


def run_edge(src, op):
    """Image.sobel and its siblings with the gate check: the expected kernel family, and no other."""
    with gated() as g:
        got = getattr(Image.new_from_array(src), op)().numpy()
    ran, convs = families(g.report)
    if src.dtype == np.uint8:
        assert ran == {"edge_u8": 1} and convs == 0, (op, src.dtype, g.report)
    else:
        assert ran == {"edge_combine_f32": 1} and convs == 2, (op, src.dtype, g.report)
    return got


def check_edge(src, op, what=""):
    want = Ref.run(op, src)
    assert want.dtype == np.uint8
    same(run_edge(src, op), want, "%s %s on %s %s" % (op, what, src.shape, src.dtype))


# ---- the fused uchar kernel

@pytest.mark.parametrize("op", EDGES)
def test_edge_uchar_tiny(op):
    """Images where every pel is an edge pel, every band count, noise and a constant."""
    for bands in BANDS:
        for width, height in TINY:
            check_edge(noise(width, height, bands, np.uint8, 3 + bands), op, "noise")
            check_edge(np.full((height, width, bands), 200, np.uint8), op, "constant")


@pytest.mark.parametrize("bands", BANDS)
def test_sobel_uchar_sizes_round_the_tile(bands):
    """Every width x height round the tile: T - 1, T, T + 1, 2 T + 5 (the odd widths of 1 and 3 bands have strides
    that are no multiple of 4)."""
    widths, heights = round_the_tile(bands)
    assert any((w * bands) % 4 for w in widths) or bands == 4
    for width in widths:
        for height in heights:
            check_edge(noise(width, height, bands, np.uint8, 21 + bands), "sobel", "noise")


@pytest.mark.parametrize("op", ["scharr", "prewitt"])
def test_scharr_prewitt_uchar_round_the_tile(op):
    """The other two masks on the corners of that cross."""
    for bands in BANDS:
        widths, heights = round_the_tile(bands)
        for width, height in ((widths[0], heights[2]), (widths[2], heights[0]), (widths[3], heights[3])):
            check_edge(noise(width, height, bands, np.uint8, 25 + bands), op, "noise")


@pytest.mark.parametrize("op", EDGES)
def test_edge_uchar_patterns(op):
    """The structured inputs, at one tile + 1 and at an odd small size."""
    tw, th = tile()
    for bands in BANDS:
        for width, height in ((-(-tw // bands) + 1, th + 1), (37, 23)):
            for name, src in sorted(patterns(width, height, bands).items()):
                check_edge(src, op, name)


def test_edge_uchar_clips_are_kept():
    """The first clip (the convolution's, to 0 .. 255) sits between the two stages and is observable: on noise some
    pels must have a convolution beyond each end, or this input shows nothing."""
    src = noise(300, 40, 1, np.uint8, 31)
    pad = np.pad(src[:, :, 0].astype(np.int64), 1, mode="edge")
    mask = np.array([[1, 2, 1], [0, 0, 0], [-1, -2, -1]])
    conv = sum(mask[j, i] * pad[j:j + 40, i:i + 300] for j in range(3) for i in range(3))
    assert (conv > 2 * 127 + 1).any() and (conv < -2 * 128 - 1).any()
    check_edge(src, "sobel", "clips")


# ---- the general tier

def ranged(w, h, bands, dtype, seed):
    """Noise of a small range, so that gradients land inside 0 .. 255 and the square root's rounding and the cast's
    truncation show; signed formats cross zero."""
    v = noise(w, h, bands, np.uint8, seed).astype(np.int64) % 61
    if np.dtype(dtype).kind == "i":
        v = v - 30
    if np.dtype(dtype).kind == "f":
        return (v.astype(np.float32) * np.float32(0.37)).astype(dtype)
    return v.astype(dtype)


@pytest.mark.parametrize("dtype", [np.int8, np.uint16, np.int16, np.int32, np.uint32, np.float32],
                         ids=lambda d: np.dtype(d).name)
def test_sobel_formats(dtype):
    """Every other format: two float convolutions and the combine, on full-range noise (which saturates the cast),
    small-range noise and the tiny sizes."""
    tw, th = tile()
    for bands in (1, 3):
        at = -(-(tw // 4) // bands)  # (elements of these formats are not the fused kernel's bytes: any size will do)
        for width, height in ((at + 1, th + 1), (2, 2), (1, 1), (7, 1), (1, 7)):
            check_edge(noise(width, height, bands, dtype, 41 + bands), "sobel", "noise")
            check_edge(ranged(width, height, bands, dtype, 45 + bands), "sobel", "small range")


@pytest.mark.parametrize("op", ["scharr", "prewitt"])
def test_scharr_prewitt_float(op):
    """The summation order of a rotated mask is its own: scharr's and prewitt's masks on float noise with fractions."""
    for bands in BANDS:
        src = (noise(131, 19, bands, np.float32, 51 + bands) * np.float32(0.013)).astype(np.float32)
        check_edge(src, op, "fractions")
        check_edge(ranged(67, 9, bands, np.int16, 55), op, "short")


def uchar_combine(c1, c2):
    """vips_edge_uchar_gen, edge.c:96-104."""
    v = np.abs(2 * (c1.astype(np.int32) - 128)) + np.abs(2 * (c2.astype(np.int32) - 128))
    return np.minimum(v, 255).astype(np.uint8)


def test_uchar_general_tier():
    """With the Highway arithmetic of convi selected (it rounds negative sums another way than the C path) the fused
    kernel steps aside: the two convolutions of vips_hip_conv as they then are, and the uchar combine."""
    src = noise(200, 30, 3, np.uint8, 61)
    mask = np.array([[1.0, 2.0, 1.0], [0.0, 0.0, 0.0], [-1.0, -2.0, -1.0]])
    mask90 = np.ascontiguousarray(np.rot90(mask, -1))
    assert Ref.run("rot", mask[:, :, None], "angle=d90")[:, :, 0].tolist() == mask90.tolist()
    lib.vips_hip_vector_set_enabled(1)
    try:
        im = Image.new_from_array(src)
        with gated() as g:
            got = im.sobel().numpy()
        c1 = im.conv(mask, scale=2.0, offset=128.0, precision="integer").numpy()
        c2 = im.conv(mask90, scale=2.0, offset=128.0, precision="integer").numpy()
    finally:
        lib.vips_hip_vector_set_enabled(0)
    ran, convs = families(g.report)
    assert ran == {"edge_combine_u8": 1} and convs == 2, g.report
    same(got, uchar_combine(c1, c2), "general tier on uchar")
    # and the C path's two convolutions, composed the same way, are the fused kernel's pixels
    c1 = im.conv(mask, scale=2.0, offset=128.0, precision="integer").numpy()
    c2 = im.conv(mask90, scale=2.0, offset=128.0, precision="integer").numpy()
    same(run_edge(src, "sobel"), uchar_combine(c1, c2), "fused against conv + conv + combine")


# ---- the region form

RECTS = ((20, 15, 40, 30), (0, 0, 17, 9), (70, 55, 20, 15), (0, 60, 90, 10), (85, 0, 5, 70))


def region_pair(src, rect, halo, out_dtype):
    """An input window that only just covers what the output rect (left, top, w, h) reads, and the output."""
    H, W = src.shape[:2]
    left, top, w, h = rect
    x0, y0 = max(left - halo, 0), max(top - halo, 0)
    x1, y1 = min(left + w + halo, W), min(top + h + halo, H)
    win = Image.new_from_array(np.ascontiguousarray(src[y0:y1, x0:x1]))
    rin = win.region()
    rin.left, rin.top, rin.im_width, rin.im_height = x0, y0, W, H
    out = Image.new_from_array(np.zeros((h, w, src.shape[2]), out_dtype))
    rout = out.region()
    rout.left, rout.top, rout.im_width, rout.im_height = left, top, W, H
    return win, rin, out, rout


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float32], ids=lambda d: np.dtype(d).name)
def test_edge_region_form(dtype):
    """An output rect strictly inside the image and rects touching every edge, from an input window that only just
    holds the halo, against the same rect of the whole-image result."""
    src = noise(90, 70, 3, dtype, 71) if dtype == np.uint8 else ranged(90, 70, 3, dtype, 71)
    for edge, op in enumerate(EDGES):
        whole = run_edge(src, op)
        for rect in RECTS:
            win, rin, out, rout = region_pair(src, rect, 1, np.uint8)
            with gated() as g:
                _ffi.check(lib.vips_hip_edge_gen(ctypes.byref(rin), ctypes.byref(rout), edge))
                got = out.numpy()
            ran, _ = families(g.report)
            assert ran == ({"edge_u8": 1} if dtype == np.uint8 else {"edge_combine_f32": 1}), g.report
            left, top, rw, rh = rect
            same(got, np.ascontiguousarray(whole[top:top + rh, left:left + rw]), "%s region %r" % (op, rect))
    # a window that does not hold the halo
    win, rin, out, rout = region_pair(src, RECTS[0], 0, np.uint8)
    lib.vips_hip_error_clear()
    assert lib.vips_hip_edge_gen(ctypes.byref(rin), ctypes.byref(rout), 0) == -1
    assert "input region too small" in _ffi.error_buffer()
    lib.vips_hip_error_clear()


def test_edge_need_rule():
    top, rows = ctypes.c_int(), ctypes.c_int()
    for at, n in ((16, 16), (0, 5), (100, 1)):
        lib.vips_hip_edge_need(at, n, ctypes.byref(top), ctypes.byref(rows))
        assert (top.value, rows.value) == (at - 1, n + 2)


# ---- refusals

def test_edge_refusals():
    """What the device does not take is refused by name: no other path runs it."""
    for op in EDGES:
        with pytest.raises(VipsHipError, match=op + ": double images"):
            getattr(Image.new_from_array(noise(40, 30, 1, np.float64, 81)), op)()
    src = noise(20, 10, 2, np.uint8, 82)
    win, rin, out, rout = region_pair(src, (0, 0, 20, 10), 1, np.uint16)
    lib.vips_hip_error_clear()
    assert lib.vips_hip_edge_gen(ctypes.byref(rin), ctypes.byref(rout), 0) == -1
    assert "sobel: the output is uchar" in _ffi.error_buffer()
    lib.vips_hip_error_clear()
    assert lib.vips_hip_edge_gen(ctypes.byref(rin), ctypes.byref(rout), 3) == -1
    assert "edge should be" in _ffi.error_buffer()
    lib.vips_hip_error_clear()


def test_wide_pels_take_the_general_tier():
    """A pel wider than the fused kernel's tile holds: the convolutions and the uchar combine, the same answer."""
    bands = lib.vips_hip_edge_step(2) + 1
    src = noise(bands * 5, 4, 1, np.uint8, 91).reshape(4, 5, bands)
    with gated() as g:
        got = Image.new_from_array(src).sobel().numpy()
    ran, convs = families(g.report)
    assert ran == {"edge_combine_u8": 1} and convs == 2, g.report
    same(got, Ref.run("sobel", src), "%d bands" % bands)


# ---- compass

KIRSCH = np.array([[5.0, 5.0, 5.0], [-3.0, 0.0, -3.0], [-3.0, -3.0, -3.0]])
LOP3 = np.array([[1.0, 2.0, -1.0], [3.0, 0.0, -2.0], [0.0, -4.0, 1.0]])  # no symmetry: eight distinct turns
MASK5 = (np.arange(25.0).reshape(5, 5) % 7) - 3.0
ANGLES = ["d0", "d45", "d90", "d135", "d180", "d225", "d270", "d315"]
COMBINES = ["max", "min", "sum"]


def compass_args(times, angle, combine, precision):
    return "times=%d,angle=%s,combine=%s,precision=%s" % (times, angle, combine, precision)


def run_compass(src, mask, times, angle, combine, precision, fused, scale=1.0, offset=0.0):
    with gated() as g:
        got = Image.new_from_array(src).compass(mask, times=times, angle=angle, combine=combine, precision=precision,
                                                scale=scale, offset=offset).numpy()
    ran = {k: n for k, (n, _) in g.report.items() if k.startswith("compass_") or k.startswith("edge_")}
    convs = sum(n for k, (n, _) in g.report.items() if k.startswith("conv"))
    if fused:
        assert ran == {"compass_u8": 1} and convs == 0, g.report
    else:
        assert ran == {"compass_combine": 1}, g.report
        if precision != "approximate":  # (what a vips_conva launches is its own affair)
            period = 8 // np.gcd(8, ANGLES.index(angle)) if angle != "d0" else 1
            assert convs == min(times, period), g.report
    return got


def check_compass(src, mask, times=2, angle="d90", combine="max", precision="float", fused=False, scale=1.0, offset=0.0):
    want = Ref.run_mask("compass", src, mask, scale, offset, args=compass_args(times, angle, combine, precision))
    got = run_compass(src, mask, times, angle, combine, precision, fused, scale, offset)
    same(got, want, "compass %s x%d %s %s on %s %s" % (angle, times, combine, precision, src.shape, src.dtype))


@pytest.mark.parametrize("combine", COMBINES)
def test_compass_fused_times_and_angles(combine):
    """uchar, precision integer, 3 x 3: times 1, 2, 4, 8 and 9 (one past the longest period) x every angle, on an
    image of one tile + 1 -- the multiplicity of a mask shows in the sum only."""
    tw, th = tile()
    src = noise(-(-tw // 3) + 1, th + 1, 3, np.uint8, 101)
    for times in (1, 2, 4, 8, 9):
        for angle in ANGLES:
            check_compass(src, LOP3, times, angle, combine, "integer", fused=True)


@pytest.mark.parametrize("bands", BANDS)
def test_compass_fused_sizes(bands):
    """The fused kernel round the tile and on the tiny sizes, the uint output of the sum included; a scale and an
    offset that drive both clips."""
    widths, heights = round_the_tile(bands)
    sizes = [(widths[0], heights[2]), (widths[1], heights[1]), (widths[2], heights[0]), (widths[3], heights[3])] + TINY
    for width, height in sizes:
        src = noise(width, height, bands, np.uint8, 105 + bands)
        check_compass(src, KIRSCH, 8, "d45", "max", "integer", fused=True)
        check_compass(src, KIRSCH, 9, "d45", "sum", "integer", fused=True, scale=3.0, offset=100.0)
        check_compass(src, LOP3, 3, "d135", "min", "integer", fused=True, scale=2.0, offset=128.0)


def test_compass_fused_patterns():
    for name, src in sorted(patterns(67, 21, 3).items()):
        check_compass(src, KIRSCH, 8, "d45", "max", "integer", fused=True, scale=4.0)
        check_compass(src, KIRSCH, 1000, "d90", "sum", "integer", fused=True)


@pytest.mark.parametrize("precision", ["integer", "float", "approximate"])
def test_compass_general_precisions(precision):
    """The general tier: a 5 x 5 mask in every precision, a 3 x 3 one where the fused kernel does not apply, the three
    combines."""
    src = noise(150, 20, 3, np.uint8, 111)
    for combine in COMBINES:
        check_compass(src, MASK5, 4, "d45", combine, precision, scale=5.0, offset=3.0)
        if precision != "integer":
            check_compass(src, LOP3, 9, "d135", combine, precision)


@pytest.mark.parametrize("dtype", [np.int8, np.uint16, np.int16, np.int32, np.float32], ids=lambda d: np.dtype(d).name)
def test_compass_general_formats(dtype):
    """Every other format with precision integer (the format is kept: abs of the format's minimum stays itself) and
    float; the float sum's order of addition shows on noise with fractions."""
    src = noise(97, 18, 2, dtype, 115)
    if np.dtype(dtype).kind == "f":
        src = (src * np.float32(0.37)).astype(np.float32)
    for combine in COMBINES:
        check_compass(src, LOP3, 9, "d45", combine, "float")
        check_compass(ranged(97, 18, 2, dtype, 117), KIRSCH, 3, "d90", combine, "integer", scale=2.0)
    check_compass(src, LOP3, 2, "d180", "max", "integer")


def tall(width, bands, dtype, seed):
    """Four more rows than the combining kernels have in flight, a few pels wide: noise."""
    rows = lib.vips_hip_edge_step(6) + 4
    assert rows > lib.vips_hip_edge_step(6) > 0
    return np.ascontiguousarray(helpers.lcg_image(width, rows, bands, dtype, seed))


@pytest.mark.parametrize("dtype", [np.uint8, np.int16, np.float32], ids=lambda d: np.dtype(d).name)
def test_edge_combine_second_turn(dtype):
    """More rows than grid.y of edge_combine_f32 (short and float images, against the reference) and of edge_combine_u8:
    a block's second row.  edge_combine_u8 runs for uchar under the Highway arithmetic, which the scalar reference does
    not have: as in test_uchar_general_tier its result is compared with the library's own two convolutions under that
    arithmetic combined in numpy (edge.c:96-104), so this case checks the combine, not the convolutions; the fused
    kernel on the same tall image is then compared with the reference."""
    src = tall(3, 1, dtype, 131)
    if dtype != np.uint8:
        check_edge(src, "sobel", "second turn")
        return
    want = Ref.run("sobel", src)
    lib.vips_hip_vector_set_enabled(1)
    try:
        im = Image.new_from_array(src)
        with gated() as g:
            got = im.sobel().numpy()
        c1 = im.conv(np.array([[1.0, 2.0, 1.0], [0.0, 0.0, 0.0], [-1.0, -2.0, -1.0]]), scale=2.0, offset=128.0, precision="integer").numpy()
        c2 = im.conv(np.array([[-1.0, 0.0, 1.0], [-2.0, 0.0, 2.0], [-1.0, 0.0, 1.0]]), scale=2.0, offset=128.0, precision="integer").numpy()
    finally:
        lib.vips_hip_vector_set_enabled(0)
    ran, convs = families(g.report)
    assert ran == {"edge_combine_u8": 1} and convs == 2, g.report
    same(got, uchar_combine(c1, c2), "general tier on uchar, second turn")
    # (the reference's own C path rounds a negative sum another way: where no sum is negative before the offset the
    # two agree, and everywhere the fused kernel is the reference)
    same(run_edge(src, "sobel"), want, "fused, tall")


@pytest.mark.parametrize("combine", COMBINES)
def test_compass_combine_second_turn(combine):
    """More rows than grid.y of compass_combine: a block's second row."""
    check_compass(tall(4, 2, np.int16, 133), LOP3, 3, "d45", combine, "float")


def test_compass_defaults_and_errors():
    src = noise(60, 30, 3, np.uint8, 121)
    want = Ref.run_mask("compass", src, KIRSCH)
    same(Image.new_from_array(src).compass(KIRSCH).numpy(), want, "defaults")
    # an even or non-square mask: vips_rot45's message, as the reference gives it
    for bad in (np.ones((2, 2)), np.ones((3, 5)), np.ones((4, 4))):
        with pytest.raises(VipsHipError, match="rot45: images must be odd and square"):
            Image.new_from_array(src).compass(bad)
        with pytest.raises(RuntimeError, match="images must be odd and square"):
            Ref.run_mask("compass", src, bad)
    with pytest.raises(VipsHipError, match="compass: double images"):
        Image.new_from_array(noise(40, 30, 1, np.float64, 122)).compass(KIRSCH)


@pytest.mark.parametrize("case", [(np.uint8, "integer", 3), (np.uint8, "float", 3), (np.uint16, "integer", 5)],
                         ids=lambda c: "%s-%s-%d" % (np.dtype(c[0]).name, c[1], c[2]))
def test_compass_region_form(case):
    dtype, precision, size = case
    mask = np.ascontiguousarray(LOP3 if size == 3 else MASK5)
    src = noise(90, 70, 3, dtype, 131)
    fused = dtype == np.uint8 and precision == "integer" and size == 3
    for combine in ("max", "sum"):
        whole = run_compass(src, mask, 3, "d45", combine, precision, fused)
        plan = _ffi.check_handle(lib.vips_hip_compass_new(mask.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), size, size,
                                                          1.0, 0.0, 3, 1, libvips_amd.image.COMBINES[combine],
                                                          libvips_amd.image.PRECISIONS[precision], 5, 1))
        try:
            assert lib.vips_hip_compass_out_format(plan, libvips_amd.image.DTYPE_FORMATS[np.dtype(dtype)]) == \
                libvips_amd.image.DTYPE_FORMATS[whole.dtype]
            for rect in RECTS:
                win, rin, out, rout = region_pair(src, rect, size // 2, whole.dtype)
                with gated() as g:
                    _ffi.check(lib.vips_hip_compass_gen(plan, ctypes.byref(rin), ctypes.byref(rout)))
                    got = out.numpy()
                assert ("compass_u8" if fused else "compass_combine") in g.report
                left, top, rw, rh = rect
                same(got, np.ascontiguousarray(whole[top:top + rh, left:left + rw]), "compass region %r" % (rect,))
            win, rin, out, rout = region_pair(src, RECTS[0], 0, whole.dtype)
            lib.vips_hip_error_clear()
            assert lib.vips_hip_compass_gen(plan, ctypes.byref(rin), ctypes.byref(rout)) == -1
            assert "input region too small" in _ffi.error_buffer()
            lib.vips_hip_error_clear()
        finally:
            lib.vips_hip_compass_free(plan)


# ---- canny

def canny_tile():
    t = tuple(lib.vips_hip_edge_step(i) for i in (3, 4))
    assert all(v > 0 for v in t), t
    return t


def run_canny(src, sigma, precision, kernel):
    """Image.canny with the gate check; the float kernel's marginal count comes back beside the pixels."""
    libvips_amd.canny_marginal()
    with gated() as g:
        got = Image.new_from_array(src).canny(sigma=sigma, precision=precision).numpy()
    ran = {k: n for k, (n, _) in g.report.items() if k.startswith("canny_")}
    assert ran == {kernel: 1}, g.report
    return got, libvips_amd.canny_marginal()


def check_canny(src, sigma=1.4, precision="float", what=""):
    """Equality with the reference, and beside it the guarantee it rests on: no pel of the float kernel sat within
    4 ulp of a rounding boundary of theta (the integer kernel has no such spot)."""
    want = Ref.run("canny", src, "sigma=%g,precision=%s" % (sigma, precision))
    uchar = want.dtype == np.uint8
    assert uchar == (src.dtype == np.uint8 and (precision != "float" or sigma < 0.2))
    got, marginal = run_canny(src, sigma, precision, "canny_polar_thin_u8" if uchar else "canny_polar_thin_f32")
    assert marginal == 0, "%d marginal pels: pick another input" % marginal
    same(got, want, "canny sigma %g %s %s on %s %s" % (sigma, precision, what, src.shape, src.dtype))


def canny_sizes(bands):
    tw, th = canny_tile()
    return [(tw - 1, th + 1), (tw, th), (tw + 1, th - 1), (2 * tw + 5, 2 * th + 5)] + TINY


@pytest.mark.parametrize("bands", BANDS)
def test_canny_uchar_integer(bands):
    """uchar with precision integer: the integer kernel, round the tile and where every pel is an edge pel."""
    for width, height in canny_sizes(bands):
        check_canny(noise(width, height, bands, np.uint8, 141 + bands), 1.4, "integer", "noise")
    for sigma in (0.5, 3.0):
        check_canny(noise(70, 20, bands, np.uint8, 145), sigma, "integer", "noise")
    check_canny(noise(70, 20, bands, np.uint8, 146), 0.1, "integer", "no blur: full-range gradients")
    check_canny(noise(70, 20, bands, np.uint8, 146), 1.4, "approximate", "noise")


@pytest.mark.parametrize("bands", BANDS)
def test_canny_float_default(bands):
    """uchar with the default precision: the blur makes a float image, the float kernel runs."""
    for width, height in canny_sizes(bands):
        check_canny(noise(width, height, bands, np.uint8, 151 + bands), 1.4, "float", "noise")
    for sigma in (0.5, 3.0):
        check_canny(noise(70, 20, bands, np.uint8, 155), sigma, "float", "noise")
    check_canny(noise(70, 20, bands, np.uint8, 156), 0.1, "float", "no blur: the image stays uchar")


@pytest.mark.parametrize("precision", ["integer", "float"])
def test_canny_patterns(precision):
    """The step, the ramps (exact G == low ties in the thinning, where the order of operations shows), the disc, the
    constant image (atan2(0, 0))."""
    for bands in (1, 3):
        for name, src in sorted(patterns(131, 37, bands).items()):
            for sigma in (0.5, 1.4, 3.0):
                check_canny(src, sigma, precision, name)


@pytest.mark.parametrize("dtype", [np.float32, np.uint16, np.int16, np.int32], ids=lambda d: np.dtype(d).name)
def test_canny_other_formats(dtype):
    """float and ushort input (and the signed ones) take the float kernel whatever the precision; with precision
    integer the blur keeps the format and the gradient reads it as convf does."""
    for bands in (1, 3):
        src = ranged(67, 19, bands, dtype, 161 + bands)
        check_canny(src, 1.4, "float", "small range")
        if np.dtype(dtype).kind != "f":
            check_canny(src, 1.4, "integer", "small range")
        check_canny(noise(67, 19, bands, dtype, 165), 0.5, "float", "noise")


def test_canny_region_form():
    """vips_hip_canny_gen on windows of the blurred image that only just hold the halo: two pels above and to the
    left, one below and to the right."""
    top, rows = ctypes.c_int(), ctypes.c_int()
    lib.vips_hip_canny_need(16, 8, ctypes.byref(top), ctypes.byref(rows))
    assert (top.value, rows.value) == (14, 11)
    src = noise(90, 70, 3, np.uint8, 171)
    for precision, kernel in (("integer", "canny_polar_thin_u8"), ("float", "canny_polar_thin_f32")):
        whole, marginal = run_canny(src, 1.4, precision, kernel)
        assert marginal == 0
        blurred = Image.new_from_array(src).gaussblur(1.4, precision=precision).numpy()
        H, W = blurred.shape[:2]
        for rect in RECTS:
            left, top_, w, h = rect
            x0, y0 = max(left - 2, 0), max(top_ - 2, 0)
            x1, y1 = min(left + w + 1, W), min(top_ + h + 1, H)
            win = Image.new_from_array(np.ascontiguousarray(blurred[y0:y1, x0:x1]))
            rin = win.region()
            rin.left, rin.top, rin.im_width, rin.im_height = x0, y0, W, H
            out = Image.new_from_array(np.zeros((h, w, 3), whole.dtype))
            rout = out.region()
            rout.left, rout.top, rout.im_width, rout.im_height = left, top_, W, H
            with gated() as g:
                _ffi.check(lib.vips_hip_canny_gen(ctypes.byref(rin), ctypes.byref(rout)))
                got = out.numpy()
            assert kernel in g.report
            same(got, np.ascontiguousarray(whole[top_:top_ + h, left:left + w]), "canny region %r" % (rect,))
        assert libvips_amd.canny_marginal() == 0
        # a window one row short above
        left, top_, w, h = RECTS[0]
        win = Image.new_from_array(np.ascontiguousarray(blurred[top_ - 1:top_ + h + 1, left - 2:left + w + 1]))
        rin = win.region()
        rin.left, rin.top, rin.im_width, rin.im_height = left - 2, top_ - 1, W, H
        out = Image.new_from_array(np.zeros((h, w, 3), whole.dtype))
        rout = out.region()
        rout.left, rout.top, rout.im_width, rout.im_height = left, top_, W, H
        lib.vips_hip_error_clear()
        assert lib.vips_hip_canny_gen(ctypes.byref(rin), ctypes.byref(rout)) == -1
        assert "canny: input region too small" in _ffi.error_buffer()
        lib.vips_hip_error_clear()


def test_canny_refusals():
    with pytest.raises(VipsHipError, match="canny: double images"):
        Image.new_from_array(noise(40, 30, 1, np.float64, 181)).canny()
    bands = lib.vips_hip_edge_step(5) + 1
    with pytest.raises(VipsHipError, match="canny: pels of %d bands" % bands):
        Image.new_from_array(noise(bands * 6, 5, 1, np.uint8, 182).reshape(5, 6, bands)).canny()


# ---- the libvips module

import os  # noqa: E402

# (on host fibers the library under test is not the one the module was linked against)
needs_module = pytest.mark.skipif(not helpers.have_module() or bool(os.environ.get("VIPS_HIP_LIBRARY")),
                                  reason="host/_build missing, or another build of the library is under test")


@needs_module
@pytest.mark.parametrize("strips", [False, True], ids=["whole", "strips"])
def test_module_edge_classes(strips):
    """sobel_hip, scharr_hip, prewitt_hip, compass_hip and canny_hip make the built-in operations' pixels, whole and
    strip by strip (a small $VIPS_HIP_BUDGET, as tests/test_module.py)."""
    Ref.load_module()
    module = ctypes.CDLL(helpers.MODULE_LIB)
    height = 900 if strips else 60
    src = helpers.lcg_image(500, height, 3, np.uint8, 191)
    wide = (helpers.lcg_image(500, height, 1, np.uint16, 192) % 300).astype(np.uint16)
    if strips:
        os.environ["VIPS_HIP_BUDGET"] = "300k"
    before = module.vips_hip_module_strips_done()
    libvips_amd.canny_marginal()
    try:
        for op in EDGES:
            same(Ref.run(op + "_hip", src), Ref.run(op, src), op + "_hip")
        same(Ref.run("sobel_hip", wide), Ref.run("sobel", wide), "sobel_hip ushort")
        for args in ("times=8,angle=d45,combine=max,precision=integer", "times=3,angle=d135,combine=sum,precision=integer",
                     "times=2,angle=d90,combine=min,precision=float"):
            same(Ref.run_mask("compass_hip", src, KIRSCH, args=args), Ref.run_mask("compass", src, KIRSCH, args=args),
                 "compass_hip " + args)
        same(Ref.run_mask("compass_hip", wide, MASK5, args="times=4,angle=d45"),
             Ref.run_mask("compass", wide, MASK5, args="times=4,angle=d45"), "compass_hip ushort 5x5")
        for args in ("sigma=1.4,precision=integer", "sigma=1.4", "sigma=3,precision=float"):
            same(Ref.run("canny_hip", src, args), Ref.run("canny", src, args), "canny_hip " + args)
        same(Ref.run("canny_hip", wide, "sigma=0.5"), Ref.run("canny", wide, "sigma=0.5"), "canny_hip ushort")
    finally:
        if strips:
            del os.environ["VIPS_HIP_BUDGET"]
    if strips:
        assert module.vips_hip_module_strips_done() - before >= 12 * 2, "not strip-mined"


@needs_module
def test_module_edge_errors_and_refusals():
    """The original's words for a mask vips_rot45 refuses; double images go to the original operation."""
    Ref.load_module()
    src = noise(40, 30, 3, np.uint8, 193)
    with pytest.raises(RuntimeError, match="images must be odd and square"):
        Ref.run_mask("compass_hip", src, np.ones((4, 4)))
    wide = noise(40, 30, 1, np.float64, 194)
    for op in EDGES:
        same(Ref.run(op + "_hip", wide), Ref.run(op, wide), op + "_hip double")
    same(Ref.run("canny_hip", wide), Ref.run("canny", wide), "canny_hip double")
    same(Ref.run_mask("compass_hip", wide, KIRSCH), Ref.run_mask("compass", wide, KIRSCH), "compass_hip double")
