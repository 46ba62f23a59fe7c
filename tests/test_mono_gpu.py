"""GPU parity: greyscale on the device -- the B_W / GREY16 / RGB16 routes of vips_hip_colourspace, the new colour
steps in region form, the grey tables, and the thumbnails of images with fewer than three bands.  Everything is
compared bit for bit with the compiled reference (tests/golden/mono.npz made from it, and oracle/_ref itself where
it is present): every new path is integer, table or separately rounded float arithmetic, so there is no tolerance.
Runs on the CPU too, under the host-fiber emulation (tests/test_mono.py)."""
import ctypes
import os

import numpy as np
import pytest

import libvips_amd
from libvips_amd import Image, _ffi
from tests import helpers
from tests.golden import make_mono_golden as mono
from tests.helpers import Ref

pytestmark = pytest.mark.gpu

GOLD = np.load(os.path.join(helpers.GOLDEN, "mono.npz"))
needs_ref = pytest.mark.skipif(not helpers.have_ref(), reason="oracle/_ref missing")
needs_module = pytest.mark.skipif(not helpers.have_module(), reason="oracle/_ref or host/_build missing")

STEPS = {"sRGB2scRGB": 0, "sRGB2scRGB16": 9, "scRGB2BW": 10, "scRGB2BW16": 11, "BW2sRGB": 12, "GREY162RGB16": 13,
         "sRGB2RGB16": 14, "RGB162sRGB": 15}


@pytest.fixture(scope="module", autouse=True)
def _init():
    libvips_amd.init(0)


def same(got, want, what=""):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, got.dtype, want.shape, want.dtype)
    g = np.ascontiguousarray(got).view(np.uint8)
    w = np.ascontiguousarray(want).view(np.uint8)
    if not np.array_equal(g, w):
        bad = np.argwhere(np.ascontiguousarray(got) != np.ascontiguousarray(want))
        first = tuple(bad[0]) if len(bad) else None
        raise AssertionError("%s: %d elements differ, first at %r: got %r, want %r" % (
            what, len(bad), first, got[first] if first else None, want[first] if first else None))


def hip_colourspace(src, tag, space):
    out = Image.new_from_array(src, interpretation=tag).colourspace(space)
    return out.numpy(), mono.INTERP[out.interpretation]


def check_golden(name, got, interp):
    same(got, GOLD[name], name)
    assert interp == int(GOLD[name + "#interp"]), (name, interp)


# ---- 1. every new pair, without and with an extra band

@pytest.mark.parametrize("case", mono.pair_cases(), ids=[c[0] for c in mono.pair_cases()])
def test_pair_matches_golden(case):
    name, a, b, extra, seed = case
    got, interp = hip_colourspace(mono.space_input(a, 37, 29, extra, seed), a, b)
    assert interp == mono.INTERP[b]
    check_golden(name, got, interp)


@needs_ref
@pytest.mark.parametrize("case", mono.pair_cases(), ids=[c[0] for c in mono.pair_cases()])
def test_pair_matches_reference_odd_size(case):
    """1003 x 517: the width is no multiple of 4 or 16 and the rows of the one-band images are not 16-byte aligned."""
    name, a, b, extra, seed = case
    src = mono.space_input(a, 1003, 517, extra, seed + 100)
    want, want_interp = Ref.run_interp("colourspace", src, "space=" + b, mono.INTERP[a])
    got, interp = hip_colourspace(src, a, b)
    same(got, want, name)
    assert interp == want_interp == mono.INTERP[b]


@needs_ref
@pytest.mark.parametrize("pair", [("srgb", "b-w"), ("srgb", "grey16"), ("rgb16", "b-w"), ("rgb16", "grey16"),
                                  ("scrgb", "b-w"), ("scrgb", "grey16"), ("b-w", "grey16"), ("grey16", "b-w"),
                                  ("xyz", "b-w"), ("lab", "grey16"), ("labs", "b-w")],
                         ids=lambda p: "%s-%s" % p)
def test_fast_kernels_match_reference(pair):
    """1024 x 300: rows on 16-byte boundaries, the width a multiple of 16 -- the 4-pixels-per-lane kernel of the
    three-band sources and the vector path of the table kernel."""
    a, b = pair
    src = mono.space_input(a, 1024, 300, 0, 433)
    want, want_interp = Ref.run_interp("colourspace", src, "space=" + b, mono.INTERP[a])
    got, interp = hip_colourspace(src, a, b)
    same(got, want, str(pair))
    assert interp == want_interp


# ---- 2. the grey tables over every value, and the tag cases

def test_every_uchar_grey_to_grey16():
    src = np.arange(256, dtype=np.uint8).reshape(16, 16, 1)
    got, interp = hip_colourspace(src, "b-w", "grey16")
    assert interp == mono.INTERP["grey16"] and got.dtype == np.uint16
    # pinned without the reference too: the 8-bit decode then the 16-bit encode of the same curve
    assert got[0, 0, 0] == 0 and got[15, 15, 0] == 65535 and np.all(np.diff(got.reshape(-1).astype(np.int64)) > 0)
    if helpers.have_ref():
        same(got, Ref.run("colourspace", src, "space=grey16", mono.INTERP["b-w"]), "b-w -> grey16")


@needs_ref
def test_every_ushort_grey16_to_grey():
    src = np.arange(65536, dtype=np.uint16).reshape(256, 256, 1)
    got, interp = hip_colourspace(src, "grey16", "b-w")
    assert interp == mono.INTERP["b-w"]
    same(got, Ref.run("colourspace", src, "space=b-w", mono.INTERP["grey16"]), "grey16 -> b-w")


@pytest.mark.parametrize("case", mono.TAG_CASES, ids=[c[0] for c in mono.TAG_CASES])
def test_the_tag_decides_the_depth(case):
    name, bands, tag, space = case
    src = mono.tag_input(bands)
    got, interp = hip_colourspace(src, tag, space)
    check_golden(name, got, interp)
    if helpers.have_ref():
        want, want_interp = Ref.run_interp("colourspace", src, "space=" + space, mono.INTERP[tag])
        same(got, want, name)
        assert interp == want_interp
        # ... and under the 16-bit tag the same pixels give something else
        if space in ("b-w", "grey16"):
            other = "rgb16" if bands == 3 else "grey16"
            if other != space:
                assert not np.array_equal(hip_colourspace(src, other, space)[0], got)


@needs_ref
@pytest.mark.parametrize("space", ["b-w", "grey16"])
def test_the_tag_decides_the_depth_in_the_fused_kernel(space):
    """The same on rows the 4-pixels-per-lane kernel takes: ushort tagged srgb is clipped to 8 bits there too."""
    src = helpers.lcg_image(64, 16, 3, np.uint16, 472)
    src[::2] >>= 8
    got, interp = hip_colourspace(src, "srgb", space)
    want, want_interp = Ref.run_interp("colourspace", src, "space=" + space, mono.INTERP["srgb"])
    same(got, want, space)
    assert interp == want_interp


# ---- 3. special values into the grey encoders

@pytest.mark.parametrize("space", ["b-w", "grey16"])
def test_special_values_to_grey(space):
    src = mono.special_input()
    got, interp = hip_colourspace(src, "scrgb", space)
    check_golden("special|" + space, got, interp)
    if helpers.have_ref():
        same(got, Ref.run("colourspace", src, "space=" + space, mono.INTERP["scrgb"]), space)
    # the same values through the one-pixel-per-lane kernel (an extra band keeps the image off the fused one)
    with_alpha = np.concatenate([src, np.full(src.shape[:2] + (1,), 0.5, np.float32)], axis=2)
    got4, _ = hip_colourspace(with_alpha, "scrgb", space)
    assert np.array_equal(got4[:, :, :1], got)


# ---- 4. region form

WINDOWS = ((20, 15, 40, 30), (0, 0, 17, 9), (70, 55, 20, 15), (0, 60, 90, 10))
# step -> (input space, output dtype, colour bands out, the reference's operation)
REGION_STEPS = {
    "scRGB2BW": ("scrgb", np.uint8, 1, ("scRGB2BW", "")),
    "scRGB2BW16": ("scrgb", np.uint16, 1, ("scRGB2BW", "depth=16")),
    "BW2sRGB": ("b-w", np.uint8, 3, ("colourspace", "space=srgb")),
    "GREY162RGB16": ("grey16", np.uint16, 3, ("colourspace", "space=rgb16")),
    "sRGB2RGB16": ("srgb", np.uint16, 3, ("colourspace", "space=rgb16")),
    "RGB162sRGB": ("rgb16", np.uint8, 3, ("colourspace", "space=srgb")),
}


@needs_ref
@pytest.mark.parametrize("step", sorted(REGION_STEPS))
@pytest.mark.parametrize("extra", [0, 1])
def test_region_form_of_the_new_steps(step, extra):
    """vips_hip_colour_gen on four windows of a 90 x 70 image (an input window that only just covers the output
    rectangle, rectangles on every edge), and a window that is too small."""
    lib = _ffi.lib
    space, out_dtype, out_colour, (ref_op, ref_args) = REGION_STEPS[step]
    src = mono.space_input(space, 90, 70, extra, 490)
    want = Ref.run(ref_op, src, ref_args, mono.INTERP[space])
    assert want.dtype == out_dtype and want.shape[2] == out_colour + extra
    for (left, top, w, h) in WINDOWS:
        x0, y0 = max(left - 3, 0), max(top - 2, 0)
        x1, y1 = min(left + w + 3, 90), min(top + h + 2, 70)
        win = Image.new_from_array(np.ascontiguousarray(src[y0:y1, x0:x1]))
        rin = win.region()
        rin.left, rin.top, rin.im_width, rin.im_height = x0, y0, 90, 70
        out = Image.new_from_array(np.zeros((h, w, want.shape[2]), want.dtype))
        rout = out.region()
        rout.left, rout.top, rout.im_width, rout.im_height = left, top, 90, 70
        if extra:
            # the extra band's rescale, max_alpha after / before (colour.c:257-273): scRGB is 0 .. 1
            scale = {"scRGB2BW": 255.0, "scRGB2BW16": 65535.0}.get(step, 1.0)
            one = (ctypes.c_int * 1)(STEPS[step])
            _ffi.check(lib.vips_hip_colour_route_gen(one, 1, ctypes.c_double(scale), ctypes.byref(rin), ctypes.byref(rout)))
        else:
            _ffi.check(lib.vips_hip_colour_gen(STEPS[step], ctypes.byref(rin), ctypes.byref(rout)))
        same(out.numpy(), np.ascontiguousarray(want[top:top + h, left:left + w]), str((step, left, top)))
    win = Image.new_from_array(np.ascontiguousarray(src[15:45, 20:60]))
    rin = win.region()
    rin.left, rin.top, rin.im_width, rin.im_height = 20, 15, 90, 70
    lib.vips_hip_error_clear()
    assert lib.vips_hip_colour_gen(STEPS[step], ctypes.byref(rin), ctypes.byref(rout)) == -1
    assert "input region too small" in _ffi.error_buffer()
    lib.vips_hip_error_clear()


def test_route_gen_checks_the_shape_of_a_grey_route():
    lib = _ffi.lib
    src = Image.new_from_array(mono.space_input("srgb", 20, 10, 0, 491))
    rin = src.region()
    steps = (ctypes.c_int * 2)(STEPS["sRGB2scRGB"], STEPS["scRGB2BW"])
    for bands, dtype, message in ((3, np.uint8, "extra bands"), (1, np.uint16, "format")):
        out = Image.new_from_array(np.zeros((10, 20, bands), dtype))
        rout = out.region()
        lib.vips_hip_error_clear()
        assert lib.vips_hip_colour_route_gen(steps, 2, 1.0, ctypes.byref(rin), ctypes.byref(rout)) == -1
        assert message in _ffi.error_buffer(), _ffi.error_buffer()
    steps = (ctypes.c_int * 2)(STEPS["scRGB2BW"], STEPS["BW2sRGB"])
    lib.vips_hip_error_clear()
    assert lib.vips_hip_colour_route_gen(steps, 2, 1.0, ctypes.byref(rin), ctypes.byref(rin)) == -1
    assert "cannot sit at position" in _ffi.error_buffer(), _ffi.error_buffer()
    lib.vips_hip_error_clear()


# ---- 5. the pairs this library leaves out

@pytest.mark.parametrize("pair", mono.BARRED, ids=["%s-%s" % p for p in mono.BARRED])
@pytest.mark.parametrize("extra", [0, 1])
def test_barred_pairs_have_no_route(pair, extra):
    a, b = pair
    with pytest.raises(libvips_amd.VipsHipError, match="no known route"):
        Image.new_from_array(mono.space_input(a, 20, 20, extra, 492), interpretation=a).colourspace(b)


# ---- 6. launch counts

@pytest.mark.parametrize("pair,kernel", [(("b-w", "grey16"), "grey_lut_u8_u16"), (("grey16", "b-w"), "grey_lut_u16_u8"),
                                         (("srgb", "b-w"), "colour_grey_x4"), (("srgb", "grey16"), "colour_grey_x4"),
                                         (("rgb16", "b-w"), "colour_grey_x4")], ids=lambda p: "-".join(p) if isinstance(p, tuple) else p)
def test_one_launch(pair, kernel):
    a, b = pair
    lib = _ffi.lib
    src = mono.space_input(a, 256, 64, 0, 493)
    im = Image.new_from_array(src, interpretation=a)
    warm = im.colourspace(b).numpy()  # (makes the tables)
    lib.vips_hip_gate_reset()
    lib.vips_hip_gate_enable(1)
    try:
        got = im.colourspace(b).numpy()
        report = libvips_amd.gate_report()
    finally:
        lib.vips_hip_gate_enable(0)
        lib.vips_hip_gate_reset()
    assert list(report) == [kernel], report
    assert report[kernel][0] == 1, report
    assert np.array_equal(got, warm)


# ---- 7. thumbnails of images with fewer than three bands

@pytest.mark.parametrize("case", mono.THUMB_CASES, ids=[c[0] for c in mono.THUMB_CASES])
def test_grey_thumbnails(case):
    name, (w, h, bands, dtype, tag), args = case
    src = mono.thumb_input(case)
    kw = {}
    for item in args.split(","):
        k, v = item.split("=")
        kw[k] = {"true": True}.get(v, v) if k in ("linear", "crop", "size") else int(v)
    out = Image.new_from_array(src, interpretation=tag).thumbnail_image(**kw)
    got, interp = out.numpy(), mono.INTERP[out.interpretation]
    assert got.dtype == np.uint8 and interp == mono.INTERP["b-w"]
    check_golden(name, got, interp)
    if helpers.have_ref():
        want, want_interp = Ref.run_interp("thumbnail_image", src, args, mono.INTERP[tag])
        same(got, want, name)
        assert interp == want_interp


def test_linear_thumbnail_of_a_greyscale_jpeg(tmp_path):
    """Image.thumbnail() forwards to the same function: a one-band JPEG with linear=True goes through GREY16 now."""
    zz = pytest.importorskip("tests.test_zz_jpeg")
    if not zz._ref_has_jpeg():
        pytest.skip("oracle/_ref built without libjpeg")
    path = str(tmp_path / "grey.jpg")
    zz.make_jpeg(path, 1000, 750, grey=True)
    want, _ = zz.cli_thumbnail(tmp_path, path, "150x150", ("--linear",))
    out = Image.thumbnail(path, 150, 150, linear=True)
    got = out.numpy()
    assert out.interpretation == "b-w"
    same(got, want, "linear grey jpeg")


# ---- 8. the libvips module

@needs_module
@pytest.mark.parametrize("which,args", [("rgb", "space=b-w"), ("rgb", "space=grey16"), ("grey", "space=srgb"),
                                         ("rgba", "space=b-w")])
@pytest.mark.parametrize("strips", [False, True], ids=["whole", "strips"])
def test_module_colourspace_hip(which, args, strips):
    """colourspace_hip makes the built-in operation's pixels for the new spaces: the output's band count differs
    from the input's, whole and strip by strip (a small $VIPS_HIP_BUDGET, as tests/test_module_stream.py)."""
    Ref.load_module()
    module = ctypes.CDLL(helpers.MODULE_LIB)
    height = 900 if strips else 120
    src, tag = {"rgb": (helpers.lcg_image(700, height, 3, np.uint8, 494), "srgb"),
                "rgba": (helpers.lcg_image(700, height, 4, np.uint8, 495), "srgb"),
                "grey": (helpers.lcg_image(700, height, 1, np.uint8, 496), "b-w")}[which]
    want, want_interp = Ref.run_interp("colourspace", src, args, mono.INTERP[tag])
    if strips:
        os.environ["VIPS_HIP_BUDGET"] = "300k"
    before = module.vips_hip_module_strips_done()
    try:
        got, interp = Ref.run_interp("colourspace_hip", src, args, mono.INTERP[tag])
    finally:
        if strips:
            del os.environ["VIPS_HIP_BUDGET"]
    if strips:
        assert module.vips_hip_module_strips_done() - before >= 3, "not strip-mined"
    same(got, want, "%s %s" % (which, args))
    assert interp == want_interp
