"""GPU parity: vips_mapim and vips_xyz (libvips_amd/csrc/mapim.hip, interp_device.h, ops_mapim.cpp).

Every comparison is np.array_equal on the bytes, with dtype, shape and interpretation, against the compiled reference
run through its command line on .v files: `vips mapim in.v out.v index.v --interpolate .. --extend .. --background ..`.
The reference's answer does not depend on its tiles or its thread count, so there is nothing to replay.  Every case
asserts by the gate report which mapim_ kernel ran and that exactly one launch was made for images without alpha; the
launches of the premultiply chain are counted apart.

Kept out of the inputs: a NaN in the FIRST pel of an index rect handed to the bounds pass (the reference's answer there
is its machine's), NaN and infinities in float images.  Runs on the CPU too, on host fibers (tests/test_emul_mapim.py)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import libvips_amd
from libvips_amd import Image, VipsHipError, _ffi
from tests import helpers

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not helpers.have_ref(), reason="oracle/_ref not built")]

lib = _ffi.lib
VIPS = os.path.join(helpers.ROOT, "oracle", "_ref", "bin", "vips")
INTERPOLATORS = ("nearest", "bilinear", "bicubic")
EXTENDS = ("black", "copy", "repeat", "mirror", "white", "background")
INDEX_DTYPES = [np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32, np.float32, np.complex64, np.float64, np.complex128]
IMAGE_DTYPES = [np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32, np.float32]
MULTIBAND, B_W, SRGB, RGB16, GREY16 = 0, 1, 22, 25, 26
W, H = 53, 37    # the large source
SW, SH = 11, 9   # the small one
SENTINEL = 0xA5
name_of = lambda d: np.dtype(d).name  # noqa: E731


@pytest.fixture(scope="module", autouse=True)
def _init():
    libvips_amd.init(0)


class gated(object):
    """with gated() as g: ...; g.ran: {gate name: launches} of the mapim_ kernels that ran inside, g.others: of
    everything else."""

    def __enter__(self):
        lib.vips_hip_gate_reset()
        lib.vips_hip_gate_enable(1)
        self.ran = self.others = None
        return self

    def __exit__(self, *exc):
        try:
            if exc[0] is None:
                report = {k: n for k, (n, _) in libvips_amd.gate_report().items()}
                self.ran = {k: n for k, n in report.items() if k.startswith("mapim_")}
                self.others = {k: n for k, n in report.items() if not k.startswith("mapim_")}
        finally:
            lib.vips_hip_gate_enable(0)
            lib.vips_hip_gate_reset()
        return False


def same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    g, w = (a.view(np.uint8).reshape(a.shape + (-1,)) for a in (np.ascontiguousarray(got), np.ascontiguousarray(want)))
    if not np.array_equal(g, w):
        bad = np.argwhere((g != w).any(-1))
        raise AssertionError("%s: %d of %d differ, first at %s: got %r want %r" % (
            what, len(bad), got.size, bad[0], got[tuple(bad[0])], want[tuple(bad[0])]))


def vec(v):
    return " ".join(repr(float(x)) for x in np.atleast_1d(v))


def run_vips(args):
    r = subprocess.run([VIPS] + args, env=helpers.ref_cli_env(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if r.returncode != 0:
        raise RuntimeError(r.stderr.strip() or "vips %s failed" % args[0])


def ref_mapim(tmp_path, src, interp, index, interpolate="bilinear", extend="background", background=0, premultiplied=False):
    """-> (array, interpretation) of the reference's `vips mapim`; RuntimeError with its words."""
    a, b, o = (str(tmp_path / n) for n in ("in.v", "index.v", "out.v"))
    helpers.write_v(a, src, interp)
    helpers.write_v(b, index, MULTIBAND)
    args = ["mapim", a, o, b, "--interpolate", interpolate, "--extend", extend, "--background", vec(background)]
    run_vips(args + (["--premultiplied"] if premultiplied else []))
    return helpers.read_v(o)


def dev_mapim(src, interp, index, **kw):
    out = Image.new_from_array(src, interp).mapim(Image.new_from_array(index), **kw)
    return out.numpy(), lib.vips_hip_image_get_interpretation(out._h)


def check(tmp_path, src, interp, index, what, alpha_chain=False, **kw):
    """One mapim on the device against the reference: bytes, header, the kernel that ran."""
    want, want_interp = ref_mapim(tmp_path, src, interp, index, **kw)
    with gated() as g:
        got, got_interp = dev_mapim(src, interp, index, **kw)
    what = "%s: %s %s through %s %s, %r" % (what, src.shape, src.dtype, index.shape, index.dtype, kw)
    same(got, want, what)
    assert got_interp == want_interp, (what, got_interp, want_interp)
    assert g.ran == {"mapim_" + kw.get("interpolate", "bilinear"): 1}, (what, g.ran)
    if not alpha_chain:
        assert g.others == {}, (what, g.others)
    return got, g


_cache = {}


def source(w, h, bands, dtype=np.uint8, seed=5):
    """Seeded noise over the format's range (float: +- 300 with fractions), made once, never changed."""
    key = (w, h, bands, np.dtype(dtype), seed)
    if key not in _cache:
        rng = np.random.default_rng(seed)
        dt = np.dtype(dtype)
        if dt.kind in "ui":
            info = np.iinfo(dt)
            a = rng.integers(info.min, info.max, (h, w, bands), dtype=dt, endpoint=True)
        else:
            a = ((rng.random((h, w, bands)) - 0.5) * 600.0).astype(dt)
        a.setflags(write=False)
        _cache[key] = a
    return _cache[key]


def as_index(x, y, dtype):
    """Two planes of numbers as an index image of this format (complex: one band, the real part x)."""
    dt = np.dtype(dtype)
    if dt.kind == "c":
        out = np.empty(x.shape + (1,), dt)
        out.real[:, :, 0] = x  # (not x + 1j * y: an infinity times 1j has a NaN for its real part)
        out.imag[:, :, 0] = y
        return out
    with np.errstate(invalid="ignore"):
        return np.ascontiguousarray(np.stack([x, y], axis=-1).astype(dt))


def domain_index(dtype, w, h, iw=57, ih=49):
    """An index over the whole domain of the coordinate stage for a w x h source.  Real formats: both components step
    through [-2, size + 2] in quarters at different rates, with the values whose sum with window_offset + 1 is not a
    float, the edges of the clip and the infinities; NaN at interior pels.  Integer formats: every integer of
    [-2, size + 2] that the format holds and values far outside."""
    dt = np.dtype(dtype)
    k = np.arange(iw * ih)
    if dt.kind in "ui":
        info = np.iinfo(dt)
        far = [info.min, info.max, info.max - 1, info.min + 1, 127, 128, 255, 32767, 32768, 65535, 10000000, 10000001, 2 ** 31 - 1, 2 ** 31]
        vx = [v for v in list(range(-2, w + 3)) + far if info.min <= v <= info.max]
        vy = [v for v in list(range(-2, h + 3)) + far if info.min <= v <= info.max]
        x = np.array(vx, np.int64)[k % len(vx)]
        y = np.array(vy, np.int64)[(k // 3) % len(vy)]
        return as_index(x.reshape(ih, iw), y.reshape(ih, iw), dt)
    special = [0.49999997, 1 - 2.0 ** -24, 1 - 2.0 ** -25, -1.0, np.nextafter(np.float32(-1), np.float32(-2)), -2.0 ** -30, 2.0 ** -30, 1e-40,
               np.inf, -np.inf, 1e30, -1e30, 16777216.0, 16777217.0, 0.5, 1.5, 2.5, 0.4999999999999999, 3.0000000000000004]
    vx = list(np.arange(-2, w + 2.25, 0.25)) + special + [w - 2.0 ** -20, w + 1 - 2.0 ** -18, w + 1.0, w + 0.99999999999]
    vy = list(np.arange(-2, h + 2.25, 0.25)) + special + [h - 2.0 ** -20, h + 1 - 2.0 ** -18, h + 1.0, h + 0.99999999999]
    x = np.array(vx, np.float64)[k % len(vx)]
    y = np.array(vy, np.float64)[(k // 3) % len(vy)]
    # NaN inside, never in the first pel
    x[[100, 300, 1500]] = np.nan
    y[[200, 300, 2000]] = np.nan
    return as_index(x.reshape(ih, iw), y.reshape(ih, iw), dt)


def smooth_index(w, h, iw, ih, dtype=np.float32, seed=3):
    """Coordinates over [-1.5, size + 1.5] with fractions of every kind."""
    rng = np.random.default_rng(seed * 1000 + iw * 37 + ih)
    x = rng.random((ih, iw)) * (w + 3) - 1.5
    y = rng.random((ih, iw)) * (h + 3) - 1.5
    if np.dtype(dtype).kind in "ui":
        lo = max(np.iinfo(dtype).min, -2)
        x, y = np.maximum(np.rint(x), lo), np.maximum(np.rint(y), lo)
    return as_index(x, y, dtype)


# ---- the whole domain of the coordinate stage

@pytest.mark.parametrize("extend", EXTENDS)
@pytest.mark.parametrize("interpolate", INTERPOLATORS)
@pytest.mark.parametrize("dtype", INDEX_DTYPES, ids=name_of)
def test_coordinate_stage_whole_domain(tmp_path, dtype, interpolate, extend):
    """Every index format x interpolator x extend mode with a non-zero background, over the whole domain of the
    coordinate stage."""
    check(tmp_path, source(W, H, 3), MULTIBAND, domain_index(dtype, W, H), "domain", interpolate=interpolate, extend=extend,
          background=[10, 200, 77])


def test_the_domain_index_tells_the_extend_modes_apart(tmp_path):
    """The reference itself: on the float domain index the six extend modes differ from one another on hundreds of
    pels, so a wrong fetch cannot hide."""
    outs = {e: ref_mapim(tmp_path, source(W, H, 3), MULTIBAND, domain_index(np.float32, W, H), interpolate="bicubic", extend=e,
                         background=[10, 200, 77])[0] for e in EXTENDS}
    for i, a in enumerate(EXTENDS):
        for b in EXTENDS[i + 1:]:
            n = int((outs[a] != outs[b]).any(-1).sum())
            assert n >= 100, (a, b, n)


# ---- image formats

@pytest.mark.parametrize("bands", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("dtype", IMAGE_DTYPES, ids=name_of)
def test_image_formats(tmp_path, dtype, bands):
    """Every image format with 1 .. 5 bands under the three interpolators; the integer formats hold their extremes
    side by side, so that the bicubic overshoots into the clip."""
    src = source(SW, SH, bands, dtype, seed=8).copy()
    dt = np.dtype(dtype)
    if dt.kind in "ui":
        info = np.iinfo(dt)
        src[2:6:2, :, :] = info.max
        src[3:6:2, :, :] = info.min
        src[:, 3:9:2, 0] = info.min
        src[:, 4:9:2, 0] = info.max
    index = smooth_index(SW, SH, 33, 17)
    for interpolate in INTERPOLATORS:
        check(tmp_path, src, MULTIBAND, index, "formats", interpolate=interpolate, extend="copy", background=list(range(3, 3 + bands)))


# ---- alpha

@pytest.mark.parametrize("premultiplied", [False, True])
@pytest.mark.parametrize("case", [("uint8", 4, SRGB), ("uint8", 2, B_W), ("uint16", 4, RGB16), ("uint16", 2, GREY16)],
                         ids=lambda c: "%s_%d" % (c[0], c[1]))
def test_alpha_chain(tmp_path, case, premultiplied):
    """RGBA and grey + alpha: premultiply, resample as float with the ink made for the float image, unpremultiply, cast
    back -- unless the caller says the image is premultiplied already."""
    dtype, bands, interp = case
    src = source(W, H, bands, np.dtype(dtype), seed=21)
    index = domain_index(np.float32, W, H)
    for interpolate, extend in (("bilinear", "background"), ("bicubic", "mirror"), ("nearest", "white")):
        got, g = check(tmp_path, src, interp, index, "alpha", alpha_chain=True, interpolate=interpolate, extend=extend,
                       background=[200, 100, 50, 128][:bands], premultiplied=premultiplied)
        assert got.dtype == np.dtype(dtype)
        # the image and the embed's fill pel go through premultiply; then unpremultiply and the cast back
        assert g.others == ({} if premultiplied else {"premultiply": 2, "unpremultiply": 1, "cast": 1}), g.others


# ---- index sizes round the kernel's units

def unit_sizes():
    bw, bh = lib.vips_hip_mapim_step(0), lib.vips_hip_mapim_step(1)
    widths = sorted({1, 3, 15, 16, 17, 31, 33, bw - 1, bw, bw + 1})
    heights = sorted({1, 3, 4, 5, bh - 1, bh + 1})
    return widths, heights


@pytest.mark.parametrize("dtype", [np.uint8, np.int16, np.float32, np.float64], ids=name_of)
def test_index_sizes_round_the_units(tmp_path, dtype):
    """Index widths and heights round a wave's patch and a block's, for index pels of 2, 4, 8 and 16 bytes (the grid is
    not capped: there is no larger case)."""
    assert lib.vips_hip_mapim_step(2) * lib.vips_hip_mapim_step(3) == 64
    widths, heights = unit_sizes()
    src = source(SW, SH, 3)
    for iw in widths:
        for ih in heights:
            check(tmp_path, src, MULTIBAND, smooth_index(SW, SH, iw, ih, dtype), "sizes", interpolate="bilinear", extend="mirror")


# ---- scattered gathers

@pytest.mark.parametrize("interpolate", INTERPOLATORS)
def test_permutation_and_constant_index(tmp_path, interpolate):
    """A permutation of the source's pels (every lane somewhere else) and a constant index (every lane the same pel)."""
    src = source(W, H, 3)
    perm = np.random.default_rng(4).permutation(W * H)
    index = as_index((perm % W).reshape(H, W), (perm // W).reshape(H, W), np.uint32)
    got, _ = check(tmp_path, src, MULTIBAND, index, "permutation", interpolate=interpolate)
    assert np.array_equal(got, src.reshape(-1, 3)[perm].reshape(H, W, 3))
    index = as_index(np.full((13, 70), 17.25), np.full((13, 70), 30.5), np.float32)
    check(tmp_path, src, MULTIBAND, index, "constant", interpolate=interpolate)


# ---- the region form

def upload_frame(frame):
    return Image.new_from_array(np.ascontiguousarray(frame)[:, :, None])


def in_frame(array, margin, extra):
    """`array` as a window of a larger uchar frame: -> (device frame, pointer to the array's pel (0, 0), stride)."""
    h, w, b = array.shape
    row = w * b * array.dtype.itemsize
    stride = margin + row + extra
    frame = np.full((h + 2, stride), SENTINEL, np.uint8)
    frame[1:1 + h, margin:margin + row] = array.view(np.uint8).reshape(h, row)
    dev = upload_frame(frame)
    return dev, dev.data_ptr + stride + margin, stride


def region_case():
    """-> src, index, the whole-image result's inputs: an index whose rect (5, 7, 19, 13) reads the middle of the source."""
    src = source(W, H, 3)
    iw, ih = 40, 30
    xx, yy = np.meshgrid(np.arange(iw), np.arange(ih))
    x = 14.0 + 0.61 * xx - 0.2 * yy
    y = 9.0 + 0.23 * xx + 0.5 * yy
    return src, as_index(x, y, np.float32)


@pytest.mark.parametrize("interpolate", INTERPOLATORS)
def test_region_form(interpolate):
    """vips_hip_mapim_gen on windows of larger strided frames: the rect of the whole-image result; a window exactly
    vips_hip_mapim_need large succeeds, one pel smaller on any side is "input region too small" without a gather."""
    src, index = region_case()
    whole = Image.new_from_array(src).mapim(Image.new_from_array(index), interpolate=interpolate).numpy()
    left, top, rw, rh = 5, 7, 19, 13
    args = Image.mapim_args(interpolate=interpolate)
    src_dev, src_ptr, src_stride = in_frame(src, 8, 11)
    idx_dev, idx_ptr, idx_stride = in_frame(index, 16, 20)
    ipel = index.shape[2] * index.dtype.itemsize
    r_index = _ffi.Region(idx_ptr + top * idx_stride + left * ipel, left, top, rw, rh, index.shape[1], index.shape[0], 2,
                          helpers.DTYPE_FORMATS[index.dtype], idx_stride)
    need = (ctypes.c_int * 4)()
    with gated() as g:
        _ffi.check(lib.vips_hip_mapim_need(ctypes.byref(r_index), ctypes.byref(args), W, H, need))
    assert g.ran == {"mapim_bounds": 1} and g.others == {}, (g.ran, g.others)
    nl, nt, nw, nh = list(need)
    # the rect reads the middle of the source: the need is a proper window of it
    assert 0 < nl and 0 < nt and nl + nw < W and nt + nh < H and nw > 4 and nh > 4, list(need)

    def run(wl, wt, ww, wh):
        out_stride = 3 * rw + 13
        fout = np.full((rh + 2, out_stride), SENTINEL, np.uint8)
        dout = upload_frame(fout)
        r_in = _ffi.Region(src_ptr + wt * src_stride + wl * 3, wl, wt, ww, wh, W, H, 3, 0, src_stride)
        r_out = _ffi.Region(dout.data_ptr + out_stride + 5, left, top, rw, rh, index.shape[1], index.shape[0], 3, 0, out_stride)
        with gated() as gg:
            rc = lib.vips_hip_mapim_gen(ctypes.byref(r_in), ctypes.byref(r_index), ctypes.byref(r_out), ctypes.byref(args), W, H)
        return rc, gg, dout.numpy()[:, :, 0]

    rc, g, back = run(nl, nt, nw, nh)
    _ffi.check(rc)
    assert g.ran == {"mapim_bounds": 1, "mapim_" + interpolate: 1}, g.ran
    got = back[1:1 + rh, 5:5 + 3 * rw].reshape(rh, rw, 3).copy()
    back[1:1 + rh, 5:5 + 3 * rw] = SENTINEL
    assert (back == SENTINEL).all(), "bytes outside the output window were written"
    same(got, np.ascontiguousarray(whole[top:top + rh, left:left + rw]), "region form, " + interpolate)
    for wl, wt, ww, wh in ((nl + 1, nt, nw - 1, nh), (nl, nt + 1, nw, nh - 1), (nl, nt, nw - 1, nh), (nl, nt, nw, nh - 1)):
        lib.vips_hip_error_clear()
        rc, g, back = run(wl, wt, ww, wh)
        assert rc != 0 and "input region too small" in _ffi.error_buffer(), (wl, wt, ww, wh, _ffi.error_buffer())
        assert g.ran == {"mapim_bounds": 1}, g.ran
        assert (back == SENTINEL).all()
        lib.vips_hip_error_clear()
    del src_dev, idx_dev


def test_region_form_all_ink_takes_any_window():
    """A rect whose every pel is ink: any window of the input will do, and the need says so."""
    src, _ = region_case()
    args = Image.mapim_args(background=[9, 8, 7])
    src_im = Image.new_from_array(src)
    out = Image.new_from_array(np.zeros((6, 9, 3), np.uint8))
    r_out = out.region()
    r_in = _ffi.Region(src_im.data_ptr, 0, 0, 1, 1, W, H, 3, 0, W * 3)
    index_im = Image.new_from_array(as_index(np.full((6, 9), W + 40.0), np.full((6, 9), 2.0), np.float64))
    r_index = index_im.region()
    need = (ctypes.c_int * 4)()
    _ffi.check(lib.vips_hip_mapim_need(ctypes.byref(r_index), ctypes.byref(args), W, H, need))
    assert list(need)[2:] == [0, 0], list(need)
    with gated() as g:
        _ffi.check(lib.vips_hip_mapim_gen(ctypes.byref(r_in), ctypes.byref(r_index), ctypes.byref(r_out), ctypes.byref(args), W, H))
    assert g.ran == {"mapim_bounds": 1, "mapim_bilinear": 1}, g.ran
    assert np.array_equal(out.numpy(), np.broadcast_to(np.array([9, 8, 7], np.uint8), (6, 9, 3)))


@pytest.mark.parametrize("dtype,margin,extra", [(np.uint8, 3, 2), (np.uint8, 4, 0), (np.uint16, 2, 4), (np.int16, 6, 2)],
                         ids=lambda v: name_of(v) if isinstance(v, type) else str(v))
def test_region_form_index_rows_off_their_pels(dtype, margin, extra):
    """Index rows of 2- and 4-byte pels that start on whole elements but not on whole pels: the kernels read such a pel
    element by element.  The whole input as the window: no bounds pass."""
    src = source(W, H, 3)
    index = domain_index(dtype, W, H, 21, 18)
    whole = Image.new_from_array(src).mapim(Image.new_from_array(index), interpolate="bicubic", extend="repeat").numpy()
    args = Image.mapim_args(interpolate="bicubic", extend="repeat")
    src_im = Image.new_from_array(src)
    idx_dev, idx_ptr, idx_stride = in_frame(index, margin, extra)
    out = Image.new_from_array(np.zeros((18, 21, 3), np.uint8))
    r_in, r_out = src_im.region(), out.region()
    r_index = _ffi.Region(idx_ptr, 0, 0, 21, 18, 21, 18, 2, helpers.DTYPE_FORMATS[index.dtype], idx_stride)
    with gated() as g:
        _ffi.check(lib.vips_hip_mapim_gen(ctypes.byref(r_in), ctypes.byref(r_index), ctypes.byref(r_out), ctypes.byref(args), W, H))
        need = (ctypes.c_int * 4)()
        _ffi.check(lib.vips_hip_mapim_need(ctypes.byref(r_index), ctypes.byref(args), W, H, need))
    assert g.ran == {"mapim_bicubic": 1, "mapim_bounds": 1} and g.others == {}, (g.ran, g.others)
    same(out.numpy(), whole, "index rows off their pels")
    # the index reaches beyond every edge and the extend is repeat: the whole image
    assert list(need) == [0, 0, W, H]
    del idx_dev


# ---- the capped grids' second turn

def need_of_bounds(index, in_width, in_height, args):
    """vips_hip_mapim_bounds_need (the host half, which the region tests pin) of numpy's extremes of the index."""
    with np.errstate(invalid="ignore"):
        lo, hi = np.nanmin(index.astype(np.float64), axis=(0, 1)), np.nanmax(index.astype(np.float64), axis=(0, 1))
    bounds = (ctypes.c_double * 4)(lo[0], lo[1], hi[0], hi[1])
    need = (ctypes.c_int * 4)()
    _ffi.check(lib.vips_hip_mapim_bounds_need(bounds, ctypes.byref(args), in_width, in_height, need))
    return list(need)


@pytest.mark.parametrize("case", ["rows", "pels"])
def test_bounds_second_turn(case):
    """The bounds pass beyond its grid.  rows: an index one block wide with three more rows than grid.y; pels: an index
    300 pels wider than the launch's lanes (its blocks of a row alone use up the launch, so grid.y is 1 and the second
    row is a second turn too).  Every one of the four extremes is unique and lies where only a second turn reads -- for
    pels: two past the first step of the pel loop, two in the second row -- each with a NaN beside it; the four clipped
    integers, through the need they give, are those of numpy's extremes."""
    threads, most, budget = lib.vips_hip_mapim_step(5), lib.vips_hip_mapim_step(4), lib.vips_hip_mapim_step(7)
    if case == "rows":
        width, height = 37, budget + 3
        assert -(-width // threads) == 1 and height > budget
        spots = [(budget, 5), (budget + 1, 30), (budget + 2, 0), (budget + 2, 36)]
    else:
        width, height = most * threads + 300, 2
        blocks_x = -(-width // threads)
        assert blocks_x > most and -(-budget // blocks_x) == 1 < height
        spots = [(0, most * threads + 7), (0, width - 1), (1, 5), (1, most * threads + 100)]
    rng = np.random.default_rng(181)
    index = (5000.0 + 4000.0 * rng.random((height, width, 2))).astype(np.float32)
    (ya, xa), (yb, xb), (yc, xc), (yd, xd) = spots
    index[ya, xa, 0] = 1000.25   # the least x
    index[yb, xb, 1] = 20000.75  # the greatest y
    index[yc, xc, 1] = 2000.5    # the least y
    index[yd, xd, 0] = 30000.5   # the greatest x
    for y, x in spots:
        index[y, x - 1 if x else x + 1, :] = np.nan
    args = Image.mapim_args(interpolate="bilinear")
    in_width = in_height = 1 << 20
    want = need_of_bounds(index, in_width, in_height, args)
    # (every extreme counts: without any one of them the need is another)
    for y, x in spots:
        less = index.copy()
        less[y, x] = 6000.0
        assert need_of_bounds(less, in_width, in_height, args) != want
    index_im = Image.new_from_array(index)
    r_index = index_im.region()
    need = (ctypes.c_int * 4)()
    with gated() as g:
        _ffi.check(lib.vips_hip_mapim_need(ctypes.byref(r_index), ctypes.byref(args), in_width, in_height, need))
    assert g.ran == {"mapim_bounds": 1} and g.others == {}, (g.ran, g.others)
    assert list(need) == want, (list(need), want)


def test_xyz_second_turn(tmp_path):
    """More two-pel groups than an xyz launch has lanes, odd rows (their last group is one pel): the lanes' second group
    is in another row, elsewhere in it."""
    lanes = lib.vips_hip_mapim_step(7) * lib.vips_hip_mapim_step(5)
    w = 1021
    groups = (w + 1) // 2
    h = lanes // groups + 9
    assert w % 2 and groups * h > lanes and lanes % groups
    o = str(tmp_path / "xyz.v")
    run_vips(["xyz", o, str(w), str(h)])
    want, _ = helpers.read_v(o)
    with gated() as g:
        got = Image.xyz(w, h).numpy()
    same(got, want, "xyz %d x %d" % (w, h))
    assert g.ran == {} and g.others == {"xyz": 1}, g.others


# ---- errors and refusals

def last_line(text):
    return str(text).strip().splitlines()[-1].strip()


@pytest.mark.parametrize("case", ["three_band_index", "background_length"])
def test_errors_with_the_references_words(tmp_path, case):
    src = source(SW, SH, 3)
    if case == "three_band_index":
        index, kw = np.zeros((5, 5, 3), np.float32), {}
        words = "mapim: image must be two-band or complex"
    else:
        index, kw = smooth_index(SW, SH, 5, 5), {"background": [1, 2]}
        words = "linear: vector must have 1 or 3 elements"
    with pytest.raises(RuntimeError) as ref:
        ref_mapim(tmp_path, src, MULTIBAND, index, **kw)
    assert last_line(ref.value) == words, str(ref.value)
    with gated() as g:
        with pytest.raises(VipsHipError) as info:
            dev_mapim(src, MULTIBAND, index, **kw)
    assert last_line(info.value) == words, str(info.value)
    assert g.ran == {} and g.others == {}


def test_refusals_by_name():
    """What the path does not take is refused by name before any launch."""
    index = smooth_index(SW, SH, 5, 5)
    cases = [
        (source(SW, SH, 3, np.float32).astype(np.float64), index, {}, "double images are outside the HIP path"),
        (source(SW, SH, 3, np.float32).astype(np.complex64), index, {}, "complex images are outside the HIP path"),
        (source(SW, SH, 3), np.zeros((5, 5, 2), np.complex64), {}, "a complex index of more than one band is outside the HIP path"),
        (source(SW, SH, 3), index, {"interpolate": "lbb"}, "interpolator lbb is outside the HIP path"),
    ]
    for src, idx, kw, words in cases:
        with gated() as g:
            with pytest.raises(VipsHipError) as info:
                dev_mapim(src, MULTIBAND, idx, **kw)
        assert words in str(info.value) and str(info.value).startswith("mapim:"), str(info.value)
        assert g.ran == {} and g.others == {}, (words, g.ran, g.others)


# ---- xyz

def xyz_widths():
    # one pel over what a block of the scaffold makes in a turn
    return [(1, 1), (20, 10), (lib.vips_hip_mapim_step(5) * lib.vips_hip_mapim_step(6) // 8 + 1, 3)]


@pytest.mark.parametrize("k", range(3))
def test_xyz(tmp_path, k):
    w, h = xyz_widths()[k]
    o = str(tmp_path / "xyz.v")
    run_vips(["xyz", o, str(w), str(h)])
    want, want_interp = helpers.read_v(o)
    with gated() as g:
        out = Image.xyz(w, h)
        got = out.numpy()
    same(got, want, "xyz %d x %d" % (w, h))
    assert lib.vips_hip_image_get_interpretation(out._h) == want_interp == MULTIBAND
    assert g.ran == {} and g.others == {"xyz": 1}, g.others


# ---- the taste pipeline

def test_xyz_linear_mapim_pipeline(tmp_path):
    """index = xyz; out = im.mapim(index * [1, -1] + [0, height - 1]): a vertical flip, against the same chain of the
    reference's command line -- and no pel leaves the device on the way."""
    src = source(W, H, 3)
    a, x, l1, l2, o = (str(tmp_path / n) for n in ("in.v", "xyz.v", "l1.v", "l2.v", "out.v"))
    helpers.write_v(a, src, MULTIBAND)
    run_vips(["xyz", x, str(W), str(H)])
    run_vips(["linear", x, l1, "1 -1", "0"])
    run_vips(["linear", l1, l2, "1", "0 %d" % (H - 1)])
    run_vips(["mapim", a, o, l2])
    want, _ = helpers.read_v(o)
    im = Image.new_from_array(src)
    with gated() as g:
        index = Image.xyz(im.width, im.height)
        out = im.mapim(index * [1, -1] + [0, im.height - 1])
    got = out.numpy()
    same(got, want, "pipeline")
    assert np.array_equal(got, src[::-1])
    assert g.ran == {"mapim_bilinear": 1} and g.others.pop("xyz") == 1, (g.ran, g.others)
    assert all(k.startswith("arith_") for k in g.others) and sum(g.others.values()) == 2, g.others
