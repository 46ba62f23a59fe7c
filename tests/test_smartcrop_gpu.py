"""GPU parity: vips_hist_find, vips_smartcrop and the content-driven thumbnail crops (libvips_amd/csrc/hist.hip,
attention.hip, smartcrop.cpp).

Every comparison is np.array_equal against the compiled reference: counters are integers, and a crop is a copy of
pels from a position that either is the reference's or is not.  The reference does not report where it cropped; the
position is recovered by finding its output in the input (unique on these inputs, asserted).  Two kinds of input:
plain noise, where every entropy decision is a near-tie and so pins the low bits of the host-side entropy, and a
quiet ramp with one noisy disc.  Runs on the CPU too, on host fibers (tests/test_emul_smartcrop.py)."""
import math

import numpy as np
import pytest

import libvips_amd
from libvips_amd import Image, VipsHipError, _ffi
from tests import helpers
from tests.helpers import Ref
from tests.rot_cases import write_oriented_v

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not helpers.have_ref(), reason="oracle/_ref not built")]

lib = _ffi.lib
HIST_GATE = "hist_rects"
ATTENTION_GATES = ["attention_max", "attention_score"]


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


def scene(w, h, bands, seed, cx, cy, r):
    y, x = np.mgrid[0:h, 0:w]
    base = ((x * 40) // w + (y * 30) // h + 60)[..., None] + np.zeros((1, 1, bands), int)
    noise = helpers.lcg_image(w, h, bands, np.uint8, seed).astype(int)
    blob = ((x - cx) ** 2 + (y - cy) ** 2 < r * r)[..., None]
    return np.where(blob, noise, base + noise // 32).clip(0, 255).astype(np.uint8)


def noise(w, h, bands, seed=7):
    return helpers.lcg_image(w, h, bands, np.uint8, seed)


def find_crop(src, crop):
    """Every (left, top) at which `crop` lies in `src`."""
    h, w = crop.shape[:2]
    H, W = src.shape[:2]
    if h > H or w > W:
        return []
    mask = np.ones((H - h + 1, W - w + 1), bool)
    for i in range(min(w, 6)):
        mask &= (src[:H - h + 1, i:W - w + 1 + i] == crop[0, i]).all(-1)
    return [(int(x), int(y)) for y, x in np.argwhere(mask) if np.array_equal(src[y:y + h, x:x + w], crop)]


_ref_crops = {}


def ref_smartcrop(tmp_path_factory, key, make, width, height, interesting):
    """(source array, the reference's crop, its (left, top)); asked once per case."""
    k = (key, width, height, interesting)
    if k not in _ref_crops:
        src = make()
        path = str(tmp_path_factory.mktemp("smartcrop") / "in.v")
        helpers.write_v(path, src, 22 if src.shape[2] == 3 else 1)
        want, _, _ = Ref.create("smartcrop", "input=%s,width=%d,height=%d,interesting=%s" % (path, width, height, interesting))
        at = find_crop(src, want)
        assert len(at) == 1, (k, at)
        _ref_crops[k] = (src, want, at[0])
    return _ref_crops[k]


def new_image(src):
    return Image.new_from_array(src, interpretation="srgb" if src.shape[2] == 3 else "b-w")


# ---- vips_hist_find

def sizes_round_the_step(bands):
    """Widths (pels) whose rows are 1 and 3 pels, one under / at / over the bytes a wave takes of a row in a step
    (rounded to pels), and two steps + 5 pels; heights 1, 3, one under / at / over the rows a block takes in a
    step, and three steps + 1."""
    wave_bytes, block_rows = lib.vips_hip_hist_step(0), lib.vips_hip_hist_step(1)
    assert wave_bytes == 1024 and block_rows == 4
    at = -(-wave_bytes // bands)
    widths = (1, 3, at - 1, at, at + 1, 2 * at + 5)
    heights = sorted(set((1, 3, block_rows - 1, block_rows, block_rows + 1, 3 * block_rows + 1)))
    return widths, heights


@pytest.mark.parametrize("bands", [1, 2, 3, 4])
def test_hist_find_against_the_reference(bands):
    widths, heights = sizes_round_the_step(bands)
    big = noise(widths[-1], heights[-1], bands, 7 + bands)
    for w in widths:
        for h in heights:
            src = np.ascontiguousarray(big[:h, :w])
            want = Ref.run("hist_find", src)
            with gated() as g:
                got = Image.new_from_array(src).hist_find().numpy()
            assert got.dtype == np.uint32 and got.shape == want.shape and np.array_equal(got, want), (w, h)
            assert int(got.sum()) == w * h * bands
            assert sorted(g.report) == [HIST_GATE] and g.report[HIST_GATE][0] == 1, (w, h, g.report)


@pytest.mark.parametrize("bands", [1, 2, 3, 4])
def test_hist_find_bands_and_width(bands):
    """One band at a time, and an image of halved values: the output is as wide as the largest counted value + 1
    (256 when every band is counted, whatever they hold)."""
    src = noise(203, 37, bands, 3) // 2
    src[..., 0] //= 2  # (band 0 stops at 63)
    im = Image.new_from_array(src)
    hist = im.hist_find()
    assert hist.interpretation == "histogram" and hist.format == "uint" and hist.height == 1
    want = Ref.run("hist_find", src)
    assert want.shape == (1, 256, bands) and np.array_equal(hist.numpy(), want)
    for band in range(bands):
        want = Ref.run("hist_find", src, "band=%d" % band)
        got = im.hist_find(band=band).numpy()
        assert want.shape == (1, int(src[..., band].max()) + 1, 1)
        assert got.shape == want.shape and np.array_equal(got, want), band
        assert int(got.sum()) == 203 * 37
    for band in (-2, bands):
        with pytest.raises(VipsHipError, match="band"):
            im.hist_find(band=band)


def test_hist_find_refuses_other_formats():
    for dtype in (np.uint16, np.float32, np.int8):
        with gated() as g:
            with pytest.raises(VipsHipError, match="uchar"):
                Image.new_from_array(helpers.lcg_image(9, 7, 3, dtype, 1)).hist_find()
        assert g.report == {}
    with pytest.raises(VipsHipError, match="uchar"):
        Image.new_from_array(noise(9, 7, 5)).hist_find()


def test_rectangles_against_bincount():
    """The hook the entropy search uses: six windows a launch.  Left offsets 1, 2, 3 and 5 in a 3-band image (rows
    that start on every byte of a dword), windows 1 and 2 pels wide and one row high, windows that end on the
    image's last pel."""
    src = noise(211, 67, 3, 19)
    im = Image.new_from_array(src)
    rects = [(1, 0, 1, 1), (2, 5, 2, 1), (3, 66, 1, 1), (5, 9, 2, 1), (1, 1, 1, 66), (210, 0, 1, 67),
             (2, 3, 209, 1), (3, 7, 100, 50), (5, 0, 206, 67), (0, 0, 211, 67), (17, 11, 6, 3), (209, 66, 2, 1)]
    for first in (0, 6):
        batch = rects[first:first + 6]
        with gated() as g:
            got = im.hist_rects(batch)
        assert g.report[HIST_GATE][0] == 1 and sorted(g.report) == [HIST_GATE]
        for k, (left, top, w, h) in enumerate(batch):
            window = src[top:top + h, left:left + w]
            want = np.stack([np.bincount(window[..., b].ravel(), minlength=256) for b in range(3)], axis=1)
            assert np.array_equal(got[k], want), (left, top, w, h)
    for bad in ((0, 0, 212, 1), (-1, 0, 2, 2), (0, 66, 1, 2), (0, 0, 0, 1)):
        with pytest.raises(VipsHipError, match="bad extract area"):
            im.hist_rects([bad])
    with pytest.raises(VipsHipError, match="rectangles"):
        im.hist_rects([(0, 0, 1, 1)] * 7)


def tall_image(bands, rows_of_a_step, extra):
    """21-byte rows (3 bands: they start on every byte of a dword), `extra` more of them than a launch's waves take in
    one step: noise below 200 in the first step's rows, values from 200 up -- which occur nowhere else -- in the others."""
    height = rows_of_a_step + extra
    src = noise(21 // bands, height, bands, 23 + bands) % 200
    src[rows_of_a_step:] = 200 + src[rows_of_a_step:] % 56
    return np.ascontiguousarray(src)


@pytest.mark.parametrize("bands", [3, 1])
def test_hist_find_second_turn(bands):
    """More rows than the launch has waves (a wave takes a row at a time): the counts of the values that only rows of
    the second turn hold."""
    rows_of_a_step = lib.vips_hip_hist_step(2) * lib.vips_hip_hist_step(1)
    src = tall_image(bands, rows_of_a_step, 7)
    assert src.shape[0] > rows_of_a_step and src[:rows_of_a_step].max() < 200 <= src[rows_of_a_step:].min()
    want = Ref.run("hist_find", src)
    with gated() as g:
        got = Image.new_from_array(src).hist_find().numpy()
    assert got.dtype == np.uint32 and got.shape == want.shape and np.array_equal(got, want)
    assert int(got[0, 200:].sum()) == 7 * src.shape[1] * bands
    assert sorted(g.report) == [HIST_GATE] and g.report[HIST_GATE][0] == 1, g.report


def test_rectangles_second_turn():
    """Six rectangles share a launch's blocks: each turns above a sixth of the rows (rounded down to blocks).  Windows
    with left offsets 1 and 2 that end in rows only the second turn reaches."""
    n = 6
    rows_of_a_step = lib.vips_hip_hist_step(2) // n * lib.vips_hip_hist_step(1)
    src = tall_image(3, rows_of_a_step, 9)
    height = src.shape[0]
    rects = [(0, 0, 7, height), (1, 0, 6, height), (2, 2, 5, height - 2), (0, 0, 7, rows_of_a_step), (3, 1, 1, height - 1), (0, 5, 2, height - 6)]
    assert len(rects) == n and sum(h > rows_of_a_step for _, _, _, h in rects) == 5
    im = Image.new_from_array(src)
    with gated() as g:
        got = im.hist_rects(rects)
    assert g.report[HIST_GATE][0] == 1 and sorted(g.report) == [HIST_GATE]
    for k, (left, top, w, h) in enumerate(rects):
        window = np.ascontiguousarray(src[top:top + h, left:left + w])
        want = Ref.run("hist_find", window)[0]
        assert np.array_equal(got[k], want), (left, top, w, h)


# ---- vips_smartcrop

SCENE = ("scene200", lambda: scene(200, 150, 3, 5, 150, 100, 25))
# (key, input, target width, target height, runs with attention)
CASES = [
    SCENE + (64, 64, True),
    SCENE + (199, 149, True),
    SCENE + (200, 64, True),
    SCENE + (64, 150, True),
    SCENE + (191, 141, True),
    ("scene200x1", lambda: scene(200, 150, 1, 5, 40, 110, 20), 64, 48, False),
    ("scene97", lambda: scene(97, 211, 3, 5, 30, 170, 18), 50, 60, True),
    ("scene300", lambda: scene(300, 40, 3, 5, 250, 20, 15), 64, 40, True),
    ("noise200", lambda: noise(200, 150, 3), 64, 64, True),
    ("noise131x1", lambda: noise(131, 257, 1), 31, 100, False),
    ("noise640", lambda: noise(640, 480, 3), 100, 100, True),
    # the attention search enlarges these on one axis on its way to 32 x 32
    ("scene300x20", lambda: scene(300, 20, 3, 9, 225, 15, 6), 150, 10, True),
    ("scene33", lambda: scene(33, 31, 3, 9, 24, 23, 10), 16, 15, True),
]
ATTENTION_CASES = [c for c in CASES if c[4]]


def case_id(case):
    return "%s_to_%dx%d" % (case[0], case[2], case[3])


def rounds_bound(W, H, w, h):
    s = max(math.ceil((W - w) / 8.0), math.ceil((H - h) / 8.0))
    return max(math.ceil((W - w) / s), math.ceil((H - h) / s)) if s else 0


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_smartcrop_entropy(case, tmp_path_factory):
    key, make, w, h, _ = case
    src, want, (left, top) = ref_smartcrop(tmp_path_factory, key, make, w, h, "entropy")
    with gated() as g:
        got, opts = new_image(src).smartcrop(w, h, interesting="entropy", with_options=True)
        pixels = got.numpy()
    assert (opts["left"], opts["top"]) == (left, top)
    assert pixels.shape == want.shape and np.array_equal(pixels, want)
    assert (opts["attention_x"], opts["attention_y"]) == (0, 0)
    assert sorted(g.report) == [HIST_GATE], g.report
    bound = rounds_bound(src.shape[1], src.shape[0], w, h)
    assert 1 <= g.report[HIST_GATE][0] <= bound <= 8, (g.report, bound)


def test_smartcrop_entropy_edges():
    src = scene(200, 150, 3, 5, 150, 100, 25)
    im = new_image(src)
    with gated() as g:
        got, opts = im.smartcrop(200, 150, interesting="entropy", with_options=True)
        pixels = got.numpy()
    assert (opts["left"], opts["top"]) == (0, 0) and np.array_equal(pixels, src)
    assert g.report == {}  # nothing to trim: no launch
    for w, h in ((201, 150), (200, 151), (0, 10), (10, -1)):
        for mode in ("entropy", "attention", "centre"):
            with pytest.raises(VipsHipError, match="bad extract area"):
                im.smartcrop(w, h, interesting=mode)


@pytest.mark.parametrize("case", ATTENTION_CASES, ids=case_id)
def test_smartcrop_attention(case, tmp_path_factory):
    key, make, w, h, _ = case
    src, want, (left, top) = ref_smartcrop(tmp_path_factory, key, make, w, h, "attention")
    with gated() as g:
        got, opts = new_image(src).smartcrop(w, h, interesting="attention", with_options=True)
        pixels = got.numpy()
    assert (opts["left"], opts["top"]) == (left, top)
    assert pixels.shape == want.shape and np.array_equal(pixels, want)
    for name in ATTENTION_GATES:
        assert g.report[name][0] == 1, g.report
    assert HIST_GATE not in g.report
    # where the crop is clear of the image's edges on an axis, the point found is its centre on that axis
    H, W = src.shape[:2]
    if 0 < left < W - w:
        assert opts["attention_x"] == left + w // 2
    if 0 < top < H - h:
        assert opts["attention_y"] == top + h // 2
    assert 0 <= opts["attention_x"] < W and 0 <= opts["attention_y"] < H


def test_attention_cases_reach_the_interior(tmp_path_factory):
    """The check of attention_x / attention_y above means something only if some case is interior on each axis."""
    interior_x = interior_y = 0
    for key, make, w, h, _ in ATTENTION_CASES:
        src, _, (left, top) = ref_smartcrop(tmp_path_factory, key, make, w, h, "attention")
        interior_x += 0 < left < src.shape[1] - w
        interior_y += 0 < top < src.shape[0] - h
    assert interior_x >= 1 and interior_y >= 1


@pytest.mark.parametrize("mode", ["none", "centre", "low", "high", "all"])
def test_smartcrop_positional_modes(mode, tmp_path_factory):
    src = scene(200, 150, 3, 5, 150, 100, 25)
    path = str(tmp_path_factory.mktemp("positional") / "in.v")
    helpers.write_v(path, src)
    want, _, _ = Ref.create("smartcrop", "input=%s,width=%d,height=%d,interesting=%s" % (path, 63, 41, mode))
    with gated() as g:
        got, opts = new_image(src).smartcrop(63, 41, interesting=mode, with_options=True)
        pixels = got.numpy()
    assert pixels.shape == want.shape and np.array_equal(pixels, want)
    if mode == "all":
        assert pixels.shape == src.shape
    assert (opts["left"], opts["top"]) == {"none": (0, 0), "centre": (68, 54), "low": (0, 0), "high": (137, 109),
                                           "all": (0, 0)}[mode]
    assert (opts["attention_x"], opts["attention_y"]) == (0, 0)
    assert g.report == {}


# ---- thumbnails

THUMB_W, THUMB_H = 100, 80


@pytest.fixture(scope="module")
def photo():
    return scene(517, 389, 3, 31, 400, 120, 70)


def _tail(crop, linear):
    return ",width=%d,height=%d,crop=%s" % (THUMB_W, THUMB_H, crop) + (",linear=true" if linear else "")


@pytest.mark.parametrize("linear", [False, True])
@pytest.mark.parametrize("crop", ["entropy", "attention"])
def test_thumbnail_crops(photo, tmp_path, crop, linear):
    path = str(tmp_path / "photo.v")
    helpers.write_v(path, photo)
    want, _, _ = Ref.create("thumbnail_image", "in=" + path + _tail(crop, linear))
    assert want.shape == (THUMB_H, THUMB_W, 3)
    got = Image.new_from_array(photo, interpretation="srgb").thumbnail_image(THUMB_W, THUMB_H, crop=crop, linear=linear).numpy()
    assert got.shape == want.shape and np.array_equal(got, want)
    want, _, _ = Ref.create("thumbnail", "filename=" + path + _tail(crop, linear))
    got = Image.thumbnail(path, THUMB_W, THUMB_H, crop=crop, linear=linear).numpy()
    assert got.shape == want.shape and np.array_equal(got, want)


@pytest.mark.parametrize("crop", ["entropy", "attention"])
def test_thumbnail_crops_after_autorot_and_in_batches(photo, tmp_path, crop):
    """The crop comes after the orientation is undone (thumbnail.c:989-1042)."""
    turned = write_oriented_v(str(tmp_path / "turned.v"), photo, 6)
    want6, _, _ = Ref.create("thumbnail", "filename=" + turned + _tail(crop, False))
    got = Image.thumbnail(turned, THUMB_W, THUMB_H, crop=crop, no_rotate=False)
    assert got.numpy().shape == want6.shape and np.array_equal(got.numpy(), want6)
    assert not got.has_orientation
    got = Image.new_from_file(turned).thumbnail_image(THUMB_W, THUMB_H, crop=crop, no_rotate=False)
    assert np.array_equal(got.numpy(), want6)
    plain = str(tmp_path / "plain.v")
    helpers.write_v(plain, photo[::-1].copy())
    want1, _, _ = Ref.create("thumbnail", "filename=" + plain + _tail(crop, False))
    results = Image.thumbnail_batch([turned, plain], THUMB_W, THUMB_H, crop=crop, no_rotate=False, threads=2)
    assert np.array_equal(results[0].numpy(), want6) and np.array_equal(results[1].numpy(), want1)


# ---- what stays refused

@pytest.mark.parametrize("mode", ["entropy", "attention"])
def test_refusals(mode):
    rgba = noise(90, 70, 4, 3)
    grey_alpha = noise(90, 70, 2, 3)
    ushort = helpers.lcg_image(90, 70, 3, np.uint16, 3)
    refused = [Image.new_from_array(rgba, interpretation="srgb"), Image.new_from_array(grey_alpha, interpretation="b-w"),
               Image.new_from_array(ushort, interpretation="rgb16")]
    if mode == "attention":
        refused.append(Image.new_from_array(noise(90, 70, 1, 3), interpretation="b-w"))
    for im in refused:
        with gated() as g:
            with pytest.raises(VipsHipError, match=mode):
                im.smartcrop(40, 30, interesting=mode)
        assert g.report == {}, (im.bands, im.format, g.report)
    # a thumbnail of an image with alpha says so before anything runs
    for im in refused[:2]:
        with gated() as g:
            with pytest.raises(VipsHipError, match=mode):
                im.thumbnail_image(40, 30, crop=mode)
        assert g.report == {}, (im.bands, g.report)
