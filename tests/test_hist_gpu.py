"""GPU parity: libvips/histogram on the device -- vips_maplut, vips_hist_cum, vips_hist_norm, vips_hist_equal,
vips_hist_local (CLAHE included) and vips_stdif (libvips_amd/csrc/hist.hip, hist_local.hip, ops_histogram.cpp).

Everything here is integer arithmetic, or double arithmetic on integers done in the reference's order, so every
comparison is np.array_equal against the compiled reference -- values, dtype and shape; nothing has a tolerance.  Every
case asserts by the gate report which kernel family ran and that it was launched once.  Sizes are taken round the
kernels' tiles (vips_hip_hist_step, vips_hip_hist_local_step, vips_hip_stdif_step) and kept small: the reference's
hist_local costs O(window height) an element.

The cases are sparse crosses, as in tests/test_rank_morph_gpu.py: every window x every max_slope x every band count on
an image that IS the window (every output reflects) and on one a pel larger; every size round the tile for one window a
kernel family; every kind of input for a few windows.  vips_maplut is checked against lut[min(in, n - 1)] with the band
rules of maplut.c, and the model itself against the reference (a LUT handed over as a .v file), as is the whole
hist_equal chain.

Two cases cannot be put to the compiled reference as the issue words them: its vips_stdif takes windows of up to 256 a
side (the argument's range, stdif.c:348-360), so 257 x 257 -- the largest this library takes -- is checked against a
numpy restatement of stdif.c that the other windows pin to the reference, and 256 x 256, the largest the reference
takes, against the reference.
Runs on the CPU too, on host fibers (tests/test_emul_hist.py)."""
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

BANDS = [1, 3, 4]
FAMILIES = ("hist_rects", "maplut_u8", "hist_local_", "stdif_u8")
HISTOGRAM = 10  # VipsInterpretation


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
                self.ran = {k: n for k, (n, _) in libvips_amd.gate_report().items() if k.startswith(FAMILIES)}
        finally:
            lib.vips_hip_gate_enable(0)
            lib.vips_hip_gate_reset()
        return False


_noise = {}


def noise(w, h, bands, seed=11):
    """A w x h corner of one noise image per (bands, seed): made once, never changed."""
    key = (bands, seed)
    if key not in _noise or _noise[key].shape[0] < h or _noise[key].shape[1] < w:
        have = _noise.get(key)
        side_w = max(w, have.shape[1] if have is not None else 0, 560)
        side_h = max(h, have.shape[0] if have is not None else 0, 300)
        _noise[key] = helpers.lcg_image(side_w, side_h, bands, np.uint8, seed)
    return np.ascontiguousarray(_noise[key][:h, :w])


def same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d of %d differ, first at %s: got %r want %r" % (
            what, len(bad), got.size, bad[0], got[tuple(bad[0])], want[tuple(bad[0])]))


# ---- hist_cum / hist_norm

def histograms(b):
    """Hand-made one-row histograms of b bands: from noise, everything in one bin, counts above 2^24 with different
    and with equal maxima a band (vips_linear's two loops), narrower than 256 (hist_find's band=k)."""
    out = []
    out.append(("noise", Ref.run("hist_find", noise(97, 41, b, 21 + b))))
    one = np.zeros((1, 256, b), np.uint32)
    one[0, 77, :] = 5000
    out.append(("one bin", one))
    big = (helpers.lcg_image(256, 1, b, np.uint32, 31 + b) >> 9) + np.uint32(1 << 22)  # 2^22 .. 2^23 + 2^22 a bin: sums near 2^31
    out.append(("large counts", big))
    flat = np.full((1, 256, b), (1 << 24) + 3, np.uint32)
    flat[0, 0::2, :] = (1 << 23) + 1
    out.append(("large counts, equal bands", flat))
    out.append(("narrow", np.ascontiguousarray(big[:, :10, :1])))
    out.append(("narrow, all bands", np.ascontiguousarray(big[:, :37, :])))
    return out


@pytest.mark.parametrize("b", BANDS)
def test_hist_cum_and_norm(b):
    for what, h in histograms(b):
        with gated() as g:
            cum = Image.new_from_array(h, "histogram").hist_cum()
            got_cum = cum.numpy()
            got_norm = cum.hist_norm().numpy()
            got_norm_h = Image.new_from_array(h, "histogram").hist_norm().numpy()
        assert g.ran == {}, g.ran  # host work: no kernel
        want_cum = Ref.run("hist_cum", h, interpretation=HISTOGRAM)
        same(got_cum, want_cum, "hist_cum of " + what)
        assert cum.interpretation == "histogram"
        same(got_norm, Ref.run("hist_norm", want_cum, interpretation=HISTOGRAM), "hist_norm of the cum of " + what)
        same(got_norm_h, Ref.run("hist_norm", h, interpretation=HISTOGRAM), "hist_norm of " + what)
        if what.startswith("large"):
            assert int(want_cum.max()) > 1 << 24


def test_hist_cum_refuses_other_images():
    with pytest.raises(VipsHipError, match="hist_cum: a 4 x 1 ushort image"):
        Image.new_from_array(np.ones((1, 4, 1), np.uint16)).hist_cum()
    with pytest.raises(VipsHipError, match="hist_norm: a 4 x 2 uint image"):
        Image.new_from_array(np.ones((2, 4, 1), np.uint32)).hist_norm()


# ---- hist_equal

def equal_sizes(bands):
    wave_bytes, block_rows = lib.vips_hip_hist_step(0), lib.vips_hip_hist_step(1)
    assert wave_bytes > 0 and block_rows > 0
    return ((1, 1), (17, 5), (-(-(wave_bytes + 1) // bands), block_rows + 1), (-(-(2 * wave_bytes + 1) // bands), 2 * block_rows + 1))


@pytest.mark.parametrize("bands", BANDS)
def test_hist_equal(bands):
    for width, height in equal_sizes(bands):
        srcs = {"noise": noise(width, height, bands, 41 + bands),
                "constant": np.full((height, width, bands), 7, np.uint8),
                "0 to 9": noise(width, height, bands, 45 + bands) % 10}
        # (so that band=k gives a LUT of 10 entries and the clip runs on the other bands)
        srcs["0 to 9"][..., 1:] = noise(width, height, bands, 49)[..., 1:]
        srcs["0 to 9"][0, 0, 0] = 9
        for what, src in srcs.items():
            for band in range(-1, bands):
                want = Ref.run("hist_equal", src, "band=%d" % band)
                with gated() as g:
                    got = Image.new_from_array(src).hist_equal(band=band).numpy()
                assert g.ran == {"hist_rects": 1, "maplut_u8": 1}, g.ran
                same(got, want, "hist_equal band=%d of %s %dx%dx%d" % (band, what, width, height, bands))


def test_hist_equal_refusals():
    with pytest.raises(VipsHipError, match="hist_equal: ushort images"):
        Image.new_from_array(np.ones((3, 4, 1), np.uint16)).hist_equal()
    with pytest.raises(VipsHipError, match="hist_equal: uchar images of 5 bands"):
        Image.new_from_array(np.ones((3, 4, 5), np.uint8)).hist_equal()
    with pytest.raises(VipsHipError, match="hist_equal: band must be -1, or less than 3"):
        Image.new_from_array(np.ones((3, 4, 3), np.uint8)).hist_equal(band=3)


# ---- maplut

LUT_DTYPES = [np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32, np.float32, np.float64]


def make_lut(n, bands, dtype, seed):
    dtype = np.dtype(dtype)
    raw = helpers.lcg_image(n, 1, bands, np.float32 if dtype.kind == "f" else dtype, seed)
    if dtype.kind == "f":
        raw = ((raw - np.float32(100.5)) * np.float32(3.25)).astype(dtype)
    return np.ascontiguousarray(raw)


def model_maplut(src, lut, band=-1):
    """maplut.c: PACK_TABLE (:562-581) and the three loops, the index clipped to n - 1."""
    n, lb = lut.shape[1], lut.shape[2]
    idx = np.minimum(src.astype(np.int64), n - 1)
    table = lut[0]  # (n, lb)
    if band >= 0 and lb == 1:
        ident = np.arange(n).astype(lut.dtype)
        cols = [table[:, 0] if b == band else ident for b in range(src.shape[2])]
        return np.ascontiguousarray(np.stack([cols[b][idx[..., b]] for b in range(src.shape[2])], axis=-1))
    if lb == 1:
        return np.ascontiguousarray(table[:, 0][idx])
    if src.shape[2] == 1:
        return np.ascontiguousarray(table[idx[..., 0]])
    return np.ascontiguousarray(np.stack([table[:, b][idx[..., b]] for b in range(lb)], axis=-1))


def run_maplut(src, lut, band=-1):
    with gated() as g:
        got = Image.new_from_array(src).maplut(Image.new_from_array(lut, "histogram"), band=band).numpy()
    assert g.ran == {"maplut_u8": 1}, g.ran
    return got


# (input bands, LUT bands, band)
MAPLUT_FORMS = [(3, 1, -1), (1, 3, -1), (3, 3, -1), (3, 1, 1), (1, 1, -1), (4, 4, -1), (1, 4, -1)]


@pytest.mark.parametrize("dtype", LUT_DTYPES, ids=lambda d: np.dtype(d).name)
def test_maplut_formats(dtype):
    """Every LUT format x n in 1, 10, 256 x every form of bands, on an image whose rows are 17 pels (rows that start on
    every byte of a dword)."""
    for n in (1, 10, 256):
        for ib, lb, band in MAPLUT_FORMS:
            src = noise(17, 7, ib, 51 + ib)
            lut = make_lut(n, lb, dtype, 61 + n + lb)
            same(run_maplut(src, lut, band), model_maplut(src, lut, band),
                 "maplut %s n=%d %d bands through %d, band=%d" % (np.dtype(dtype).name, n, ib, lb, band))


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float64], ids=lambda d: np.dtype(d).name)
def test_maplut_row_widths(dtype):
    """Rows of 1, 15, 16, 17 bytes and round the 1 024 bytes a wave takes in a step; strides that are no multiple of
    4; a column LUT."""
    wave = lib.vips_hip_hist_step(0)
    for ib, lb, band in ((1, 1, -1), (3, 1, -1), (1, 3, -1), (3, 3, -1), (3, 1, 2)):
        for row_bytes in (1, 15, 16, 17, 33, wave - 1, wave, wave + 1, 2 * wave + 5):
            width = max(1, row_bytes // ib)
            for height in (1, 6):
                src = noise(width, height, ib, 71 + ib)
                lut = make_lut(200, lb, dtype, 81 + lb)
                same(run_maplut(src, lut, band), model_maplut(src, lut, band),
                     "maplut rows of %d x %d bands, %d high, through %d" % (width, ib, height, lb))
    src = noise(23, 5, 3, 75)
    lut = make_lut(256, 1, dtype, 85)
    column = np.ascontiguousarray(lut.reshape(256, 1, 1))
    same(run_maplut(src, column), model_maplut(src, lut), "column LUT")


@pytest.mark.parametrize("form", [(3, 3, -1), (1, 4, -1)], ids=lambda f: "%dthrough%d" % f[:2])
def test_maplut_second_turn(tmp_path, form):
    """More rows than the launch has waves (a wave takes a row at a time), rows of 21 and 7 bytes that start on every
    byte of a dword."""
    ib, lb, band = form
    rows_of_a_step = lib.vips_hip_hist_step(3) * lib.vips_hip_hist_step(1)
    src = np.ascontiguousarray(helpers.lcg_image(7, rows_of_a_step + 7, ib, np.uint8, 91 + ib))
    assert src.shape[0] > rows_of_a_step
    lut = make_lut(256, lb, np.uint16, 93 + lb)
    path = str(tmp_path / "lut.v")
    helpers.write_v(path, lut, interpretation=HISTOGRAM)
    want = Ref.run("maplut", src, "lut=" + path)
    same(run_maplut(src, lut, band), want, "maplut second turn %r" % (form,))


def test_the_maplut_model_is_the_reference(tmp_path):
    """vips_object_set_from_string loads an image argument from a file name: the LUT goes over as a .v file."""
    cases = [(3, 1, -1, np.uint8, 256), (1, 3, -1, np.uint16, 256), (3, 3, -1, np.float32, 10), (3, 1, 1, np.int16, 10),
             (3, 1, 0, np.uint8, 1), (4, 1, -1, np.float64, 100), (1, 4, -1, np.int32, 256)]
    for k, (ib, lb, band, dtype, n) in enumerate(cases):
        src = noise(19, 6, ib, 91 + k)
        lut = make_lut(n, lb, dtype, 95 + k)
        path = str(tmp_path / ("lut%d.v" % k))
        helpers.write_v(path, lut, interpretation=HISTOGRAM)
        args = "lut=" + path + (",band=%d" % band if band >= 0 else "")
        want = Ref.run("maplut", src, args)
        same(model_maplut(src, lut, band), want, "model %r" % (cases[k],))
        same(run_maplut(src, lut, band), want, "device %r" % (cases[k],))


def test_maplut_interpretation():
    src = Image.new_from_array(noise(9, 4, 1, 99), "b-w")
    assert src.maplut(Image.new_from_array(make_lut(256, 3, np.uint8, 1), "histogram")).interpretation == "srgb"
    assert src.maplut(Image.new_from_array(make_lut(256, 3, np.uint16, 1), "srgb")).interpretation == "srgb"
    assert src.maplut(Image.new_from_array(make_lut(256, 3, np.uint16, 1), "histogram")).interpretation == "rgb16"
    assert src.maplut(Image.new_from_array(make_lut(256, 1, np.uint8, 1), "histogram")).interpretation == "b-w"
    rgb = Image.new_from_array(noise(9, 4, 3, 99), "srgb")
    assert rgb.maplut(Image.new_from_array(make_lut(256, 1, np.float32, 1), "histogram")).interpretation == "srgb"
    assert Image.new_from_array(noise(9, 4, 3, 99)).maplut(
        Image.new_from_array(make_lut(256, 1, np.uint16, 1), "histogram")).interpretation == "rgb16"
    for lut_dtype, want_tag in ((np.uint8, "histogram"), (np.uint16, "histogram")):
        row = Image.new_from_array(noise(9, 1, 1, 99), "b-w")
        assert row.maplut(Image.new_from_array(make_lut(256, 3, lut_dtype, 1), "histogram")).interpretation == want_tag
    # and the reference's
    _, interp = Ref.run_interp("hist_equal", noise(9, 4, 3, 99))
    assert Image.new_from_array(noise(9, 4, 3, 99)).hist_equal().interpretation == libvips_amd.image.INTERPRETATION_NAMES[interp]
    _, interp = Ref.run_interp("hist_equal", noise(9, 1, 1, 99))
    assert Image.new_from_array(noise(9, 1, 1, 99)).hist_equal().interpretation == libvips_amd.image.INTERPRETATION_NAMES[interp]


def test_maplut_refusals():
    im = Image.new_from_array(noise(9, 4, 3, 99))
    lut = Image.new_from_array(make_lut(256, 1, np.uint8, 1))
    with pytest.raises(VipsHipError, match="maplut: histograms must have width or height 1"):
        im.maplut(Image.new_from_array(np.zeros((2, 128, 1), np.uint8)))
    with pytest.raises(VipsHipError, match="maplut: images must have the same number of bands, or one must be single-band"):
        im.maplut(Image.new_from_array(make_lut(256, 2, np.uint8, 1)))
    with pytest.raises(VipsHipError, match="maplut: a table of 65536 entries"):
        im.maplut(Image.new_from_array(np.zeros((1, 65536, 1), np.uint16)))
    with pytest.raises(VipsHipError, match="maplut: ushort index images"):
        Image.new_from_array(np.ones((3, 4, 1), np.uint16)).maplut(lut)
    with pytest.raises(VipsHipError, match="maplut: complex tables"):
        im.maplut(Image.new_from_array(np.zeros((1, 256, 1), np.complex64)))
    with pytest.raises(VipsHipError, match="maplut: a table of 256 entries x 5 bands of double"):
        Image.new_from_array(noise(9, 4, 1, 99)).maplut(Image.new_from_array(make_lut(256, 5, np.float64, 1)))
    # the reference says the first two in the same words
    with pytest.raises(RuntimeError, match="histograms must have width or height 1"):
        Ref.run("hist_cum", np.zeros((2, 128, 1), np.uint8))


# ---- hist_local

def hl_steps():
    t = [lib.vips_hip_hist_local_step(i) for i in range(7)]
    assert all(v > 0 for v in t), t
    return dict(run=t[0], rows=t[1], side=t[2], lanes=t[3], count_area=t[4], count_elems=t[5], count_rows=t[6])


def hl_family(w, h, max_slope):
    return "hist_local_count" if max_slope == 0 and w * h <= hl_steps()["count_area"] else "hist_local_slide"


def hl_tile(family, bands):
    """(pels, rows) a block of the family makes."""
    s = hl_steps()
    if family == "hist_local_count":
        return -(-s["count_elems"] // bands), s["count_rows"]
    return (s["lanes"] // bands) * s["run"], s["rows"]


def hl_args(w, h, max_slope):
    return "width=%d,height=%d,max-slope=%d" % (w, h, max_slope)


def run_hist_local(src, w, h, max_slope):
    with gated() as g:
        got = Image.new_from_array(src).hist_local(w, h, max_slope).numpy()
    assert g.ran == {hl_family(w, h, max_slope): 1}, (w, h, max_slope, g.ran)
    return got


def check_hist_local(src, w, h, max_slope, what=""):
    want = Ref.run("hist_local", src, hl_args(w, h, max_slope))
    same(run_hist_local(src, w, h, max_slope), want, "hist_local %dx%d slope %d on %s %s" % (w, h, max_slope, src.shape, what))


SLOPES = [0, 1, 3, 100]
HL_WINDOWS = [(1, 1), (3, 3), (2, 5), (5, 2), (8, 8), (15, 17), (31, 31), (64, 64), "widest", "tallest"]


def hl_window(window):
    side = hl_steps()["side"]
    return (side, 1) if window == "widest" else (1, side) if window == "tallest" else window


@pytest.mark.parametrize("window", HL_WINDOWS, ids=lambda w: w if isinstance(w, str) else "%dx%d" % w)
def test_hist_local_windows(window):
    """Every window x every max_slope x every band count on an image that IS the window (every output reflects) and on
    one a pel larger."""
    w, h = hl_window(window)
    families = set()
    for bands in BANDS:
        for width, height in ((w, h), (w + 1, h + 1)):
            src = noise(width, height, bands, 101 + bands)
            for max_slope in SLOPES:
                check_hist_local(src, w, h, max_slope)
                families.add(hl_family(w, h, max_slope))
    assert "hist_local_slide" in families


def test_both_families_run():
    assert {hl_family(w, h, s) for (w, h) in HL_WINDOWS[:8] for s in SLOPES} == {"hist_local_count", "hist_local_slide"}
    assert hl_family(8, 8, 0) == "hist_local_count" and hl_family(8, 8, 1) == "hist_local_slide"
    assert hl_family(9, 8, 0) == "hist_local_slide"


@pytest.mark.parametrize("bands", BANDS)
def test_hist_local_sizes_round_the_tile(bands):
    """One window a family (and CLAHE) on every width x height round its tile: T - 1, T, T + 1, 2 T + 5."""
    for w, h, max_slope in ((3, 3, 0), (4, 7, 3), (11, 7, 0)):
        tw, th = hl_tile(hl_family(w, h, max_slope), bands)
        for width in (tw - 1, tw, tw + 1, 2 * tw + 5):
            for height in (th - 1, th, th + 1, 2 * th + 5):
                check_hist_local(noise(width, height, bands, 111 + bands), w, h, max_slope)


@pytest.mark.parametrize("kind", ["four values", "constant", "ramp"])
def test_hist_local_inputs(kind):
    """Noise & 0xC0 (four values: every bin far above any max_slope), a constant image, a horizontal ramp."""
    for bands in BANDS:
        width, height = 70, 21
        if kind == "four values":
            src = noise(width, height, bands, 121 + bands) & 0xC0
        elif kind == "constant":
            src = np.full((height, width, bands), 200, np.uint8)
        else:
            src = np.ascontiguousarray(np.broadcast_to((np.arange(width) * 255 // (width - 1)).astype(np.uint8)[None, :, None],
                                                       (height, width, bands)))
        for w, h in ((3, 3), (15, 17), (8, 8)):
            for max_slope in SLOPES:
                check_hist_local(src, w, h, max_slope, kind)


def test_hist_local_errors_and_refusals():
    src = noise(40, 30, 3, 131)
    im = Image.new_from_array(src)
    with pytest.raises(VipsHipError, match="hist_local: window too large"):
        im.hist_local(41, 3)
    with pytest.raises(VipsHipError, match="hist_local: window too large"):
        im.hist_local(3, 31, 2)
    with pytest.raises(RuntimeError, match="window too large"):
        Ref.run("hist_local", src, hl_args(41, 3, 0))
    with pytest.raises(RuntimeError, match="window too large"):
        Ref.run("hist_local", src, hl_args(3, 31, 0))
    with pytest.raises(VipsHipError, match="hist_local: max_slope must be 0 to 100"):
        im.hist_local(3, 3, 101)
    with pytest.raises(VipsHipError, match=r"hist_local: image must be VIPS_FORMAT_UCHAR \(it is ushort\)"):
        Image.new_from_array(np.ones((30, 40, 1), np.uint16)).hist_local(3, 3)
    with pytest.raises(RuntimeError, match="image must be VIPS_FORMAT_UCHAR"):
        Ref.run("hist_local", np.ones((30, 40, 1), np.uint16), hl_args(3, 3, 0))
    big = Image.new_from_array(noise(300, 300, 1, 133))
    with pytest.raises(VipsHipError, match="hist_local: a 256 x 256 window: .* 65535 pels"):
        big.hist_local(256, 256)
    with pytest.raises(VipsHipError, match="hist_local: a 257 x 3 window"):
        big.hist_local(257, 3, 1)
    with pytest.raises(VipsHipError, match="hist_local: a 255 x 256 window on 1-band images needs .* KB of LDS"):
        big.hist_local(255, 256)
    with pytest.raises(VipsHipError, match="hist_local: 17-band images"):
        Image.new_from_array(noise(20, 12, 17, 135)).hist_local(9, 9)


# ---- stdif

def sd_args(w, h, a=0.5, m0=128.0, b=0.5, s0=50.0):
    return "width=%d,height=%d,a=%r,m0=%r,b=%r,s0=%r" % (w, h, a, m0, b, s0)


def run_stdif(src, w, h, **kw):
    with gated() as g:
        got = Image.new_from_array(src).stdif(w, h, **kw).numpy()
    assert g.ran == {"stdif_u8": 1}, g.ran
    return got


def check_stdif(src, w, h, what="", **kw):
    want = Ref.run("stdif", src, sd_args(w, h, **kw))
    same(run_stdif(src, w, h, **kw), want, "stdif %dx%d %r on %s %s" % (w, h, kw, src.shape, what))


def model_stdif(src, w, h, a=0.5, m0=128.0, b=0.5, s0=50.0):
    """stdif.c:170-226: unsigned int sums, the doubles one operation at a time, the store as the reference's machine
    does it (a double in 256 .. 256.5 to a byte: 0)."""
    padded = np.pad(src, ((h // 2, h - 1 - h // 2), (w // 2, w - 1 - w // 2), (0, 0)), mode="edge").astype(np.uint64)

    def box(v):
        c = np.zeros((v.shape[0] + 1, v.shape[1] + 1, v.shape[2]), np.uint64)
        c[1:, 1:] = v.cumsum(0).cumsum(1)
        return (c[h:, w:] - c[:-h, w:] - c[h:, :-w] + c[:-h, :-w]) & np.uint64(0xffffffff)

    n = float(w * h)
    s, s2 = box(padded).astype(np.float64), box(padded * padded).astype(np.float64)
    mean = s / n
    var = s2 / n - mean * mean
    sig = np.sqrt(var)
    f1, f2, f3 = a * m0, 1.0 - a, b * s0
    res = (f1 + f2 * mean) + (src.astype(np.float64) - mean) * (f3 / (s0 + b * sig))
    out = ((res + 0.5).astype(np.int64) & 255)
    return np.ascontiguousarray(np.where(res < 0.0, 0, np.where(res >= 256.0, 255, out)).astype(np.uint8))


SD_WINDOWS = [(1, 1), (3, 3), (2, 5), (5, 2), (8, 8), (15, 17), (31, 31)]
SD_PARAMS = [dict(), dict(a=0.0), dict(a=1.0), dict(b=0.0), dict(b=2.0), dict(m0=0.0), dict(m0=255.7), dict(s0=1.0),
             dict(a=1.0, b=2.0, m0=255.7, s0=1.0), dict(a=0.0, b=2.0, m0=0.0, s0=1.0)]


@pytest.mark.parametrize("window", SD_WINDOWS, ids=lambda w: "%dx%d" % w)
def test_stdif_windows(window):
    w, h = window
    for bands in BANDS:
        for width, height in ((w, h), (w + 1, h + 1), (71, 23)):
            if width < w or height < h:
                continue
            src = noise(width, height, bands, 141 + bands)
            for kw in (SD_PARAMS if (width, height) == (71, 23) else SD_PARAMS[:1] + SD_PARAMS[-2:]):
                check_stdif(src, w, h, **kw)


@pytest.mark.parametrize("bands", BANDS)
def test_stdif_sizes_round_the_tile(bands):
    tw, th = -(-lib.vips_hip_stdif_step(0) // bands), lib.vips_hip_stdif_step(1)
    assert tw > 0 and th > 0
    for width in (tw - 1, tw, tw + 1, 2 * tw + 5):
        for height in (th - 1, th, th + 1, 2 * th + 5):
            check_stdif(noise(width, height, bands, 151 + bands), 5, 4, a=0.3, b=1.5)


def test_stdif_corners():
    """The store of 255.5 <= res < 256 (a constant image of 255 with a = 1, m0 = 255.7), and a sweep over noise at
    3 x 3, where sig is largest."""
    white = np.full((9, 20, 3), 255, np.uint8)
    check_stdif(white, 3, 3, "white", a=1.0, m0=255.7)
    assert int(run_stdif(white, 3, 3, a=1.0, m0=255.7)[4, 10, 1]) == 0  # 256.2 as a byte
    check_stdif(white, 3, 3, "white", a=1.0, m0=255.4)
    check_stdif(white, 5, 3, "white", a=0.0, m0=255.7)
    for seed in range(4):
        src = noise(130, 40, 3, 161 + seed)
        for kw in (dict(), dict(a=0.0, b=2.0, s0=1.0), dict(a=1.0, m0=255.7, b=2.0, s0=1.0), dict(b=2.0, m0=0.0, s0=1.0)):
            check_stdif(src, 3, 3, "noise %d" % seed, **kw)


def test_stdif_largest_windows():
    """256 x 256, the largest the reference's arguments take, against the reference; the model against the reference
    there and at 15 x 17; 257 x 257 = 66049 pels, just under this library's limit, against the model."""
    src = noise(300, 260, 1, 171)
    want = Ref.run("stdif", src, sd_args(256, 256))
    same(run_stdif(src, 256, 256), want, "stdif 256x256")
    same(model_stdif(src, 256, 256), want, "model 256x256")
    small = noise(60, 40, 3, 173)
    same(model_stdif(small, 15, 17, a=0.2, b=1.7, m0=100.0, s0=3.0), Ref.run("stdif", small, sd_args(15, 17, a=0.2, b=1.7, m0=100.0, s0=3.0)),
         "model 15x17")
    same(run_stdif(src, 257, 257), model_stdif(src, 257, 257), "stdif 257x257")
    same(run_stdif(src, 257, 257, a=1.0, b=2.0, s0=1.0), model_stdif(src, 257, 257, a=1.0, b=2.0, s0=1.0), "stdif 257x257")


def test_stdif_tall_image_guard_second_turn():
    """An 87 x 256 window on four bands leaves room in LDS for one output row a block, so a row of blocks is a row of
    the image and the grid takes 65 535 of them: one row more is refused by name, before any launch.  (The side that
    runs is not here: 131 070 blocks that each stage 256 rows of 608 bytes, and a reference of 22 M elements under a
    window of 22 272 pels, are no test of seconds; windows that leave two rows a block put the guard at 131 070 rows.)"""
    src = np.ascontiguousarray(helpers.lcg_image(87, 65536, 4, np.uint8, 181))
    with gated() as g:
        with pytest.raises(VipsHipError, match="stdif: image too large"):
            Image.new_from_array(src).stdif(87, 256)
    assert g.ran == {}, g.ran
    # two rows fewer in the window and a block makes two rows: the same image runs into no guard
    small = np.ascontiguousarray(src[:300])
    same(run_stdif(small, 87, 250), Ref.run("stdif", small, sd_args(87, 250)), "stdif 87x250")


def test_stdif_errors_and_refusals():
    src = noise(300, 260, 1, 171)
    im = Image.new_from_array(src)
    with pytest.raises(VipsHipError, match="stdif: a 258 x 257 window has 66306 pels"):
        im.stdif(258, 257)
    with pytest.raises(VipsHipError, match="stdif: window too large"):
        im.stdif(301, 3)
    with pytest.raises(VipsHipError, match="stdif: window too large"):
        im.stdif(3, 261)
    with pytest.raises(RuntimeError, match="window too large"):
        Ref.run("stdif", noise(40, 30, 1, 171), sd_args(41, 3))
    with pytest.raises(VipsHipError, match=r"stdif: image must be VIPS_FORMAT_UCHAR \(it is float\)"):
        Image.new_from_array(np.ones((30, 40, 1), np.float32)).stdif(3, 3)


# ---- the region forms

def strips_of(height, strip):
    return [(top, min(strip, height - top)) for top in range(0, height, strip)]


def run_in_strips(src, window_height, strip, gen):
    """The image cut into strips of `strip` rows, each fed exactly the rows vips_hip_rank_need names (clipped to the
    image), joined."""
    H, W, B = src.shape
    out = np.zeros_like(src)
    top_, rows_ = ctypes.c_int(), ctypes.c_int()
    for top, n in strips_of(H, strip):
        lib.vips_hip_rank_need(window_height, top, n, ctypes.byref(top_), ctypes.byref(rows_))
        y0, y1 = max(top_.value, 0), min(top_.value + rows_.value, H)
        win = Image.new_from_array(np.ascontiguousarray(src[y0:y1]))
        rin = win.region()
        rin.left, rin.top, rin.im_width, rin.im_height = 0, y0, W, H
        part = Image.new_from_array(np.zeros((n, W, B), np.uint8))
        rout = part.region()
        rout.left, rout.top, rout.im_width, rout.im_height = 0, top, W, H
        _ffi.check(gen(ctypes.byref(rin), ctypes.byref(rout)))
        out[top:top + n] = part.numpy()
    return out


@pytest.mark.parametrize("case", [(5, 4, 0), (7, 9, 3), (3, 12, 0), (16, 11, 100)], ids=lambda c: "%dx%d-%d" % c)
def test_hist_local_region_form(case):
    """Strips of 1 row, of half the window and of a tile + 1: the first and the last strip, strips that touch no edge
    while their windows do.  A reflected row always lies inside the rows vips_hip_rank_need names."""
    w, h, max_slope = case
    src = noise(45, 31, 3, 181)
    whole = run_hist_local(src, w, h, max_slope)
    th = hl_tile(hl_family(w, h, max_slope), 3)[1]
    for strip in (1, max(1, h // 2), th + 1):
        with gated() as g:
            got = run_in_strips(src, h, strip, lambda i, o: lib.vips_hip_hist_local_gen(i, o, w, h, max_slope))
        assert set(g.ran) == {hl_family(w, h, max_slope)}, g.ran
        same(got, whole, "hist_local %r in strips of %d" % (case, strip))
    # a window that does not hold the halo
    win = Image.new_from_array(np.ascontiguousarray(src[10:12]))
    rin = win.region()
    rin.left, rin.top, rin.im_width, rin.im_height = 0, 10, 45, 31
    part = Image.new_from_array(np.zeros((2, 45, 3), np.uint8))
    rout = part.region()
    rout.left, rout.top, rout.im_width, rout.im_height = 0, 10, 45, 31
    lib.vips_hip_error_clear()
    assert lib.vips_hip_hist_local_gen(ctypes.byref(rin), ctypes.byref(rout), w, h, max_slope) == -1
    assert "hist_local: input region too small" in _ffi.error_buffer()
    lib.vips_hip_error_clear()


@pytest.mark.parametrize("case", [(5, 4), (7, 9), (3, 12)], ids=lambda c: "%dx%d" % c)
def test_stdif_region_form(case):
    w, h = case
    src = noise(45, 31, 3, 183)
    whole = run_stdif(src, w, h, a=0.3, b=1.2)
    for strip in (1, max(1, h // 2), lib.vips_hip_stdif_step(1) + 1):
        with gated() as g:
            got = run_in_strips(src, h, strip, lambda i, o: lib.vips_hip_stdif_gen(i, o, w, h, 0.3, 128.0, 1.2, 50.0))
        assert set(g.ran) == {"stdif_u8"}, g.ran
        same(got, whole, "stdif %r in strips of %d" % (case, strip))


# ---- the libvips module

@needs_module
@pytest.mark.parametrize("strips", [False, True], ids=["whole", "strips"])
def test_module_hist_local_and_stdif(strips):
    """hist_local_hip and stdif_hip make the built-in operations' pixels, whole and strip by strip (a small
    $VIPS_HIP_BUDGET, as tests/test_module.py)."""
    Ref.load_module()
    module = ctypes.CDLL(helpers.MODULE_LIB)
    height = 700 if strips else 50
    src = helpers.lcg_image(400, height, 3, np.uint8, 191)
    if strips:
        os.environ["VIPS_HIP_BUDGET"] = "300k"
    before = module.vips_hip_module_strips_done()
    try:
        for args in (hl_args(3, 3, 0), hl_args(9, 11, 0), hl_args(7, 5, 3)):
            same(Ref.run("hist_local_hip", src, args), Ref.run("hist_local", src, args), "hist_local_hip " + args)
        for args in (sd_args(11, 11), sd_args(4, 7, a=0.1, b=1.9, m0=90.0, s0=5.0)):
            same(Ref.run("stdif_hip", src, args), Ref.run("stdif", src, args), "stdif_hip " + args)
    finally:
        if strips:
            del os.environ["VIPS_HIP_BUDGET"]
    if strips:
        assert module.vips_hip_module_strips_done() - before >= 5 * 2, "not strip-mined"


@needs_module
def test_module_errors_are_the_originals():
    Ref.load_module()
    src = noise(40, 30, 3, 131)
    with pytest.raises(RuntimeError, match="hist_local_hip: window too large"):
        Ref.run("hist_local_hip", src, hl_args(41, 3, 0))
    with pytest.raises(RuntimeError, match="stdif_hip: window too large"):
        Ref.run("stdif_hip", src, sd_args(3, 31))
    with pytest.raises(RuntimeError, match="hist_local_hip: image must be VIPS_FORMAT_UCHAR"):
        Ref.run("hist_local_hip", np.ones((30, 40, 1), np.uint16), hl_args(3, 3, 0))
