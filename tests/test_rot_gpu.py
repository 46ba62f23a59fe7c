"""GPU parity: vips_rot, vips_flip, vips_autorot and the auto-rotating thumbnails (libvips_amd/csrc/rot.hip).

Every operation is a permutation of pels, so every comparison is np.array_equal on the whole output, shapes included.
numpy states the permutations (tests/rot_cases.py) and the compiled reference anchors them; the thumbnails, the .v
metadata and the libvips module are compared with the reference itself.  Every kernel case asserts which kernel ran,
by the gate report.  Runs on the CPU too, on host fibers (tests/test_emul_rot.py)."""
import ctypes
import os

import numpy as np
import pytest

import libvips_amd
from libvips_amd import Image, _ffi
from tests import helpers, rot_cases
from tests.helpers import Ref
from tests.rot_cases import ANGLES, DIRECTIONS, OPS, ORIENT, PELS, pel_id, pel_size, write_oriented_v

pytestmark = pytest.mark.gpu

lib = _ffi.lib
needs_ref = pytest.mark.skipif(not helpers.have_ref(), reason="oracle/_ref not built")
# (on host fibers the library under test is not the one the module was linked against)
needs_module = pytest.mark.skipif(not helpers.have_module() or bool(os.environ.get("VIPS_HIP_LIBRARY")),
                                  reason="oracle/_ref or host/_build missing, or another build of the library is under test")


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


def run_op(im, op):
    """op: an angle, a direction, or an orientation 1 .. 8 undone through autorot."""
    if isinstance(op, int):
        im.orientation = op
        return im.autorot()
    if op in ANGLES:
        return im.rot(op)
    return im.flip(op)


def expected(a, op):
    return ORIENT[op](a) if isinstance(op, int) else OPS[op](a)


def transposes(op):
    return op in (5, 6, 7, 8) if isinstance(op, int) else op in rot_cases.TRANSPOSING


def mirrors(op):
    return op in ("d180", "horizontal", 2, 3)


def stream_gates(width, pel, op):
    """What a row-preserving operation on a fresh image (rows back to back, base on 256 bytes) runs: the stream
    kernel where rows are whole dwords and hold at least one of its 16- / 48-byte groups (a mirror: of whole pels of
    a size the kernel is compiled for; a row-permuted copy: 16 bytes), plus the general kernel for what is left of a
    row; the general kernel alone otherwise."""
    if mirrors(op) and pel not in (1, 2, 3, 4, 6, 8, 12, 16):
        return ["rot_general"]
    chunk = 48 if mirrors(op) and 16 % pel else 16
    row = width * pel
    if row % 4 == 0 and row >= chunk:
        return ["flip_stream"] + (["rot_general"] if row % chunk else [])
    return ["rot_general"]


# the five operations and the three orientations that are a turn plus a flip
ALL_OPS = ["d90", "d180", "d270", "horizontal", "vertical", 4, 5, 7]


def sizes_round_the_tile(pel):
    t = lib.vips_hip_rot_tile_side(pel)
    assert t in (32, 64)
    return (1, 3, t - 1, t, t + 1, 2 * t + 5)


@pytest.mark.parametrize("op", ALL_OPS, ids=str)
@pytest.mark.parametrize("case", PELS, ids=pel_id)
def test_every_kernel_against_numpy(case, op):
    """Widths and heights from {1, 3, T-1, T, T+1, 2T+5}, crossed (T: the tile side for the pel size), so that every
    edge of a tile is met in both axes; the quarter turns must run the tile kernel of the pel size."""
    dtype, bands = case
    pel = pel_size(dtype, bands)
    sizes = sizes_round_the_tile(pel)
    big = helpers.lcg_image(sizes[-1], sizes[-1], bands, dtype, 7 + pel)
    for w in sizes:
        for h in sizes:
            src = np.ascontiguousarray(big[:h, :w])
            with gated() as g:
                got = run_op(Image.new_from_array(src), op).numpy()
            want = expected(src, op)
            assert got.shape == want.shape and np.array_equal(got, want), (w, h)
            gates = ["rot_tile<%d>" % pel] if transposes(op) else stream_gates(w, pel, op)
            assert sorted(g.report) == sorted(gates), (w, h, g.report)


@pytest.mark.parametrize("op", ALL_OPS, ids=str)
def test_double_images_take_the_general_kernel(op):
    sizes = (1, 3, 31, 32, 33, 69)
    big = helpers.lcg_image(69, 69, 3, np.float64, 5)
    for w in sizes:
        for h in sizes:
            src = np.ascontiguousarray(big[:h, :w])
            with gated() as g:
                got = run_op(Image.new_from_array(src), op).numpy()
            want = expected(src, op)
            assert got.shape == want.shape and np.array_equal(got, want), (w, h)
            assert sorted(g.report) == (["rot_general"] if transposes(op) else sorted(stream_gates(w, 24, op))), (w, h, g.report)


@pytest.mark.parametrize("case", PELS, ids=pel_id)
def test_general_kernel_behind_the_switch(case, monkeypatch):
    """VIPS_HIP_NO_ROT_TILE / VIPS_HIP_NO_FLIP_STREAM: the one-pel-a-lane kernel on every pel size."""
    monkeypatch.setenv("VIPS_HIP_NO_ROT_TILE", "1")
    monkeypatch.setenv("VIPS_HIP_NO_FLIP_STREAM", "1")
    dtype, bands = case
    pel = pel_size(dtype, bands)
    sizes = sizes_round_the_tile(pel)
    big = helpers.lcg_image(sizes[-1], sizes[-1], bands, dtype, 11 + pel)
    for w, h in ((1, 1), (3, sizes[4]), (sizes[4], 3), (sizes[3], sizes[2]), (sizes[5], sizes[4])):
        src = np.ascontiguousarray(big[:h, :w])
        for op in ALL_OPS:
            with gated() as g:
                got = run_op(Image.new_from_array(src), op).numpy()
            want = expected(src, op)
            assert got.shape == want.shape and np.array_equal(got, want), (w, h, op)
            assert sorted(g.report) == ["rot_general"], (w, h, op, g.report)


@pytest.mark.parametrize("orientation", range(1, 9))
def test_many_tiles(orientation):
    """1031 x 517 x 3 uchar: 17 x 9 tiles, ragged in both axes, rows that start on every byte of a dword."""
    src = helpers.lcg_image(1031, 517, 3, np.uint8, 3)
    im = Image.new_from_array(src)
    im.orientation = orientation
    with gated() as g:
        out, opts = im.autorot(with_options=True)
        got = out.numpy()
    want = ORIENT[orientation](src)
    assert got.shape == want.shape and np.array_equal(got, want)
    angle, flip = rot_cases.ORIENT_ANGLE_FLIP[orientation]
    assert opts == {"angle": angle, "flip": flip}
    assert not out.has_orientation and im.orientation == orientation
    if orientation == 1:
        assert g.report == {}  # (the same pixels, shared)
    elif orientation in rot_cases.SWAPS:
        assert sorted(g.report) == ["rot_tile<3>"] and g.report["rot_tile<3>"][0] == 1, g.report  # one launch
    else:
        assert sorted(g.report) == sorted(stream_gates(1031, 3, orientation)), g.report


def rows_over_the_grid(blocks_x, extra):
    """`extra` more rows than a launch of blocks_x blocks a row has in flight."""
    in_flight = -(-lib.vips_hip_rot_step(1) // blocks_x)
    return in_flight, in_flight + extra


@pytest.mark.parametrize("op", ["d180", "vertical", "horizontal"])
@pytest.mark.parametrize("blocks", [1, 3])
def test_flip_stream_second_turn(op, blocks):
    """More rows than grid.y (the cap for rows of one block, a third of it for rows of three): a block's second row,
    whose source row with d180 and vertical is height - 1 - y.  One block: RGB uchar, 48-byte groups; three: RGBA
    uchar, 16-byte groups.  Rows end in a ragged group, which the one-pel-a-lane kernel takes -- on its second turn too."""
    threads = lib.vips_hip_rot_step(0)
    bands = 3 if blocks == 1 else 4
    group = lib.vips_hip_rot_group(1 if op == "vertical" else bands)  # (a row-permuted copy moves rows of bytes)
    assert group == (48 if bands == 3 and op != "vertical" else 16)
    # whole groups for two lanes of the last block, or a few more, then 12 bytes: whole pels, three or four
    chunks = (blocks - 1) * threads + 2
    while (chunks * group + 12) % bands:
        chunks += 1
    width = (chunks * group + 12) // bands
    in_flight, rows = rows_over_the_grid(blocks, 5 - blocks)
    assert -(-chunks // threads) == blocks and width * bands % group == 12 and rows > in_flight
    assert (blocks == 1) == (in_flight == lib.vips_hip_rot_step(1))
    src = helpers.lcg_image(width, rows, bands, np.uint8, 31 + blocks)
    with gated() as g:
        got = run_op(Image.new_from_array(src), op).numpy()
    want = expected(src, op)
    assert got.shape == want.shape and np.array_equal(got, want)
    assert {k: n for k, (n, _) in g.report.items()} == {"flip_stream": 1, "rot_general": 1}, g.report


@pytest.mark.parametrize("case", [(np.uint8, 3, "d90", 1), (np.uint16, 1, "d270", 3), (np.float32, 1, "d180", 1), (np.float64, 1, "d90", 3),
                                  (np.uint16, 4, "horizontal", 3)], ids=lambda c: "%s_x%d-%s-%dblocks" % ((np.dtype(c[0]).name,) + c[1:]))
def test_rot_general_second_turn(case, monkeypatch):
    """The one-pel-a-lane kernel with more output rows than grid.y, copying units of 1, 2, 4 and 8 bytes (odd widths
    keep the rows' starts from allowing more than the element).  For the quarter turns the output's rows are the input's
    width."""
    monkeypatch.setenv("VIPS_HIP_NO_ROT_TILE", "1")
    monkeypatch.setenv("VIPS_HIP_NO_FLIP_STREAM", "1")
    dtype, bands, op, blocks = case
    out_width = (blocks - 1) * lib.vips_hip_rot_step(0) + 41
    in_flight, out_rows = rows_over_the_grid(blocks, 5 - blocks)
    assert -(-out_width // lib.vips_hip_rot_step(0)) == blocks and out_rows > in_flight and out_width % 2
    w, h = (out_rows, out_width) if transposes(op) else (out_width, out_rows)
    src = helpers.lcg_image(w, h, bands, dtype, 37 + blocks)
    with gated() as g:
        got = run_op(Image.new_from_array(src), op).numpy()
    want = expected(src, op)
    assert got.shape == want.shape == (out_rows, out_width, bands) and np.array_equal(got, want)
    assert {k: n for k, (n, _) in g.report.items()} == {"rot_general": 1}, g.report


def test_rot_and_flip_keep_the_orientation_other_operations_drop_it():
    src = helpers.lcg_image(40, 30, 3, np.uint8, 1)
    im = Image.new_from_array(src)
    assert not im.has_orientation and im.orientation == 1
    im.orientation = 6
    assert im.rot("d90").orientation == 6 and im.fliphor().orientation == 6
    d0 = im.rot("d0")
    assert d0.orientation == 6 and np.array_equal(d0.numpy(), src)
    assert np.array_equal(im.rot90().numpy(), OPS["d90"](src)) and np.array_equal(im.rot180().numpy(), OPS["d180"](src))
    assert np.array_equal(im.rot270().numpy(), OPS["d270"](src)) and np.array_equal(im.flipver().numpy(), OPS["vertical"](src))
    assert not im.cast("uchar").has_orientation and not im.cast("ushort").has_orientation
    assert not im.extract_area(1, 1, 8, 8).has_orientation
    with pytest.raises(libvips_amd.VipsHipError, match="bad angle"):
        im.rot(7)
    with pytest.raises(libvips_amd.VipsHipError, match="bad direction"):
        im.flip(2)


# ---- the reference

ANCHORS = [(67, 41, 3, np.uint8), (33, 19, 2, np.float32)]


@needs_ref
@pytest.mark.parametrize("shape", ANCHORS, ids=lambda s: "%dx%dx%d" % s[:3])
def test_anchor_to_the_reference(shape, tmp_path):
    w, h, b, dtype = shape
    src = helpers.lcg_image(w, h, b, dtype, 21)
    for angle in ("d90", "d180", "d270"):
        want = Ref.run("rot", src, "angle=" + angle)
        assert np.array_equal(want, OPS[angle](src)), angle  # (the numpy statement is the reference's)
        got = Image.new_from_array(src).rot(angle).numpy()
        assert got.shape == want.shape and np.array_equal(got, want), angle
    for direction in ("horizontal", "vertical"):
        want = Ref.run("flip", src, "direction=" + direction)
        assert np.array_equal(want, OPS[direction](src)), direction
        got = Image.new_from_array(src).flip(direction).numpy()
        assert got.shape == want.shape and np.array_equal(got, want), direction
    for orientation in range(1, 9):
        path = write_oriented_v(str(tmp_path / ("o%d.v" % orientation)), src, orientation, 0)
        want, _, _ = Ref.create("autorot", "in=" + path)
        assert np.array_equal(want, ORIENT[orientation](src)), orientation
        im = Image.new_from_file(path)
        assert im.has_orientation and im.orientation == orientation
        got = im.autorot().numpy()
        assert got.shape == want.shape and np.array_equal(got, want), orientation


# ---- region views

def _window(image, left, top, width, height, pel):
    r = image.region()
    r.data = r.data + top * r.stride + left * pel
    r.left, r.top, r.width, r.height = left, top, width, height
    return r


@pytest.mark.parametrize("op", ["d90", "d180", "d270", "horizontal", "vertical"])
def test_region_views(op):
    """A window with an odd left edge of a 200 x 150 x 3 image (stride != width * 3), into a window of a larger
    image: the window holds the operation on the cropped array, nothing round it is touched."""
    src = helpers.lcg_image(200, 150, 3, np.uint8, 9)
    left, top, w, h = 17, 9, 101, 77
    want = OPS[op](src[top:top + h, left:left + w])
    oh, ow = want.shape[:2]
    frame = np.full((oh + 11, ow + 14, 3), 0x5a, np.uint8)
    oleft, otop = 5, 3
    im, out = Image.new_from_array(src), Image.new_from_array(frame)
    rin, rout = _window(im, left, top, w, h, 3), _window(out, oleft, otop, ow, oh, 3)
    with gated() as g:
        if op in ANGLES:
            _ffi.check(lib.vips_hip_rot_gen(ANGLES[op], ctypes.byref(rin), ctypes.byref(rout)))
        else:
            _ffi.check(lib.vips_hip_flip_gen(DIRECTIONS[op], ctypes.byref(rin), ctypes.byref(rout)))
        got = out.numpy()
    assert sorted(g.report) == (["rot_tile<3>"] if op in rot_cases.TRANSPOSING else ["rot_general"]), g.report
    frame[otop:otop + oh, oleft:oleft + ow] = want
    assert np.array_equal(got, frame)
    # a region of the wrong size is an error, not a write out of bounds
    rout.width += 1
    assert lib.vips_hip_rot_gen(1, ctypes.byref(rin), ctypes.byref(rout)) != 0
    assert "output region must be" in _ffi.error_buffer()
    lib.vips_hip_error_clear()


# ---- thumbnails

THUMB_W, THUMB_H = 100, 80


@pytest.fixture(scope="module")
def photo():
    return helpers.lcg_image(517, 389, 3, np.uint8, 31) // 2 + helpers.lcg_image(517, 389, 3, np.uint8, 32) // 4


def _thumbnail_both_ways(path, crop, no_rotate, linear=False):
    args = "filename=%s,width=%d,height=%d" % (path, THUMB_W, THUMB_H)
    if crop != "none":
        args += ",crop=" + crop
    if no_rotate:
        args += ",no_rotate=true"
    if linear:
        args += ",linear=true"
    want, _, _ = Ref.create("thumbnail", args)
    got = Image.thumbnail(path, THUMB_W, THUMB_H, crop=crop, linear=linear, no_rotate=bool(no_rotate))
    return got, want


@needs_ref
@pytest.mark.parametrize("no_rotate", [0, 1])
@pytest.mark.parametrize("crop", ["none", "centre"])
@pytest.mark.parametrize("orientation", range(1, 9))
def test_thumbnail_honours_the_orientation(photo, tmp_path, orientation, crop, no_rotate):
    path = write_oriented_v(str(tmp_path / "photo.v"), photo, orientation)
    got, want = _thumbnail_both_ways(path, crop, no_rotate)
    pixels = got.numpy()
    assert pixels.shape == want.shape and np.array_equal(pixels, want)
    if crop == "centre":
        assert pixels.shape[:2] == (THUMB_H, THUMB_W)
    # rotated: no orientation left; no_rotate: the tag stays (the reference's output still reads it)
    assert lib.vips_hip_image_get_orientation(got._h) == (orientation if no_rotate else 0)


@needs_ref
def test_thumbnail_linear_and_alpha(photo, tmp_path):
    path = write_oriented_v(str(tmp_path / "linear.v"), photo, 6)
    for crop in ("none", "centre"):
        got, want = _thumbnail_both_ways(path, crop, 0, linear=True)
        assert got.numpy().shape == want.shape and np.array_equal(got.numpy(), want), crop
    rgba = np.concatenate([photo, helpers.lcg_image(517, 389, 1, np.uint8, 33)], axis=2)
    path = write_oriented_v(str(tmp_path / "rgba.v"), rgba, 5)
    for crop in ("none", "centre"):
        got, want = _thumbnail_both_ways(path, crop, 0)
        assert got.numpy().shape == want.shape and np.array_equal(got.numpy(), want), crop


@needs_ref
@pytest.mark.parametrize("orientation", [1, 3, 6, 7])
def test_thumbnail_image_honours_the_orientation(photo, tmp_path, orientation):
    path = write_oriented_v(str(tmp_path / "photo.v"), photo, orientation)
    for crop in ("none", "centre"):
        want, _, _ = Ref.create("thumbnail_image", "in=%s,width=%d,height=%d,crop=%s" % (path, THUMB_W, THUMB_H, crop))
        got = Image.new_from_file(path).thumbnail_image(THUMB_W, THUMB_H, crop=crop, no_rotate=False)
        assert got.numpy().shape == want.shape and np.array_equal(got.numpy(), want), crop
        assert not got.has_orientation
    # the entry point without the argument does not look at the orientation
    plain = Image.new_from_file(path).thumbnail_image(THUMB_W, THUMB_H)
    assert np.array_equal(plain.numpy(), Image.new_from_array(photo, interpretation="srgb").thumbnail_image(THUMB_W, THUMB_H).numpy())


# ---- JPEG

def _ref_has_jpeg():
    if not helpers.have_ref():
        return False
    try:
        Ref.lib()
        vips = ctypes.CDLL(helpers.REF_LIB.replace("libref_shim", "libvips"))
        vips.vips_type_find.restype = ctypes.c_size_t
        vips.vips_type_find.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
        return vips.vips_type_find(b"VipsOperation", b"jpegload") != 0
    except Exception:
        return False


def _oriented_jpeg(path, width, height, orientation):
    PIL = pytest.importorskip("PIL.Image")
    y, x = np.mgrid[0:height, 0:width]
    img = np.stack([(np.sin(x / 31.0) + 1) * 127, (np.cos(y / 19.0) + 1) * 127, (2 * x + y) % 256], axis=2)
    img = (img.astype(int) + helpers.lcg_image(width, height, 3, np.uint8, 77) // 8).clip(0, 255).astype(np.uint8)
    exif = PIL.Exif()
    exif[0x0112] = orientation
    PIL.fromarray(img).save(path, quality=90, exif=exif.tobytes())
    return path


@pytest.mark.skipif(not _ref_has_jpeg(), reason="oracle/_ref built without libjpeg")
@pytest.mark.parametrize("orientation", [6, 3])
def test_jpeg_thumbnail_honours_exif(tmp_path, orientation):
    """The oracle has no libexif: what the reference would make of the file is its thumbnail of a .v that holds its
    own jpegload at the shrink-on-load factor, plus the orientation."""
    jpeg = _oriented_jpeg(str(tmp_path / "phone.jpg"), 300, 200, orientation)
    f = lib.vips_hip_thumbnail_find_jpegshrink_rotate(300, 200, 64, 0, 0, 0, 0, int(orientation in rot_cases.SWAPS))
    assert f in (1, 2, 4, 8)
    loaded, _, _ = Ref.create("jpegload", "filename=%s,shrink=%d" % (jpeg, f))
    path = write_oriented_v(str(tmp_path / "loaded.v"), loaded, orientation)
    want, _, _ = Ref.create("thumbnail", "filename=%s,width=64" % path)
    got = Image.thumbnail(jpeg, 64, no_rotate=False)
    assert got.numpy().shape == want.shape and np.array_equal(got.numpy(), want)
    assert not got.has_orientation
    assert Image.new_from_jpeg(jpeg).orientation == orientation
    kept = Image.thumbnail(jpeg, 64, no_rotate=True)
    assert kept.orientation == orientation and kept.has_orientation
    results = Image.thumbnail_batch([jpeg, jpeg], 64, no_rotate=False, threads=2)
    assert all(np.array_equal(r.numpy(), want) for r in results)
    with pytest.raises(libvips_amd.VipsHipError, match="auto-rotation"):
        Image.thumbnail(jpeg, 64)


# ---- .v round trip

def test_vfile_round_trip(tmp_path):
    src = helpers.lcg_image(83, 47, 3, np.uint8, 13)
    im = Image.new_from_array(src, interpretation="srgb")
    plain, ours = str(tmp_path / "plain.v"), str(tmp_path / "ours.v")
    im.write_to_file(ours)
    helpers.write_v(plain, src)
    assert open(ours, "rb").read() == open(plain, "rb").read()  # no orientation: header + pixels, as before
    im.orientation = 6
    im.write_to_file(ours)
    assert open(ours, "rb").read() == open(write_oriented_v(plain, src, 6), "rb").read()
    back = Image.new_from_file(ours)
    assert back.has_orientation and back.orientation == 6 and np.array_equal(back.numpy(), src)
    upright = back.autorot().numpy()
    assert np.array_equal(upright, ORIENT[6](src))
    if helpers.have_ref():
        want, _, _ = Ref.create("autorot", "in=" + ours)
        assert want.shape == upright.shape and np.array_equal(want, upright)


# ---- the libvips module

@needs_module
@pytest.mark.parametrize("shape", ANCHORS, ids=lambda s: "%dx%dx%d" % s[:3])
def test_module_rot_flip_autorot(shape, tmp_path):
    Ref.load_module()
    w, h, b, dtype = shape
    src = helpers.lcg_image(w, h, b, dtype, 41)
    for angle in ("d0", "d90", "d180", "d270"):
        assert np.array_equal(Ref.run("rot_hip", src, "angle=" + angle), Ref.run("rot", src, "angle=" + angle)), angle
    for direction in ("horizontal", "vertical"):
        assert np.array_equal(Ref.run("flip_hip", src, "direction=" + direction),
                              Ref.run("flip", src, "direction=" + direction)), direction
    for orientation in range(1, 9):
        path = write_oriented_v(str(tmp_path / ("o%d.v" % orientation)), src, orientation, 0)
        got, _, _ = Ref.create("autorot_hip", "in=" + path)
        want, _, _ = Ref.create("autorot", "in=" + path)
        assert got.shape == want.shape and np.array_equal(got, want), orientation


@needs_module
@pytest.mark.parametrize("no_rotate", [False, True])
@pytest.mark.parametrize("orientation", [1, 3, 6, 7])
def test_module_thumbnails(photo, tmp_path, orientation, no_rotate):
    Ref.load_module()
    path = write_oriented_v(str(tmp_path / "photo.v"), photo, orientation)
    tail = ",width=%d,height=%d" % (THUMB_W, THUMB_H) + (",no_rotate=true" if no_rotate else "")
    got, _, _ = Ref.create("thumbnail_hip", "filename=" + path + tail)
    want, _, _ = Ref.create("thumbnail", "filename=" + path + tail)
    assert got.shape == want.shape and np.array_equal(got, want)
    got, _, _ = Ref.create("thumbnail_image_hip", "in=" + path + tail)
    want, _, _ = Ref.create("thumbnail_image", "in=" + path + tail)
    assert got.shape == want.shape and np.array_equal(got, want)
