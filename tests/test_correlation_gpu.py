"""GPU parity: vips_fastcor and vips_spcor (libvips_amd/csrc/correlation.hip, ops_correlation.cpp), and vips_min /
vips_max of uint and int images (arith.hip's statistics scan).

Every comparison is np.array_equal on the bytes, with dtype, shape and interpretation, against the compiled reference run
through its command line on .v files with VIPS_CONCURRENCY=1: `vips fastcor in.v ref.v out.v`, `vips spcor in.v ref.v
out.v`, `vips min in.v`.  Every case asserts from the gate report which fastcor_ / spcor_ kernel ran and that it was
launched once; calls on images of one format make no other launch, the casts of mixed formats are counted apart.

Inputs are seeded noise over the format's full range, but int within +- 2^30 (the reference's `int t = a - b` overflows
beyond) and float / double at +- 300 with fractions.  NaN and infinities are kept out: a NaN's bits are the machine's.
Runs on the CPU too, on host fibers (tests/test_emul_correlation.py)."""
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
OPS = ("fastcor", "spcor")
DTYPES = [np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32, np.float32, np.float64]
SUFFIX = {np.dtype(np.uint8): "u8", np.dtype(np.int8): "s8", np.dtype(np.uint16): "u16", np.dtype(np.int16): "s16",
          np.dtype(np.uint32): "u32", np.dtype(np.int32): "s32", np.dtype(np.float32): "f32", np.dtype(np.float64): "f64"}
MULTIBAND, B_W, SRGB = 0, 1, 22
W, H = 53, 37
name_of = lambda d: np.dtype(d).name  # noqa: E731


@pytest.fixture(scope="module", autouse=True)
def _init():
    libvips_amd.init(0)


class gated(object):
    """with gated() as g: ...; g.ran: {gate name: launches} of the fastcor_ / spcor_ kernels that ran inside, g.others:
    of everything else."""

    def __enter__(self):
        lib.vips_hip_gate_reset()
        lib.vips_hip_gate_enable(1)
        self.ran = self.others = None
        return self

    def __exit__(self, *exc):
        try:
            if exc[0] is None:
                report = {k: n for k, (n, _) in libvips_amd.gate_report().items()}
                mine = lambda k: k.startswith("fastcor_") or k.startswith("spcor_")  # noqa: E731
                self.ran = {k: n for k, n in report.items() if mine(k)}
                self.others = {k: n for k, n in report.items() if not mine(k)}
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


def run_vips(args):
    r = subprocess.run([VIPS] + args, env=helpers.ref_cli_env(VIPS_CONCURRENCY="1"), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True)
    if r.returncode != 0:
        raise RuntimeError(r.stderr.strip() or "vips %s failed" % args[0])
    return r.stdout


def ref_cor(tmp_path, op, im, ref, interp=MULTIBAND):
    """-> (array, interpretation) of the reference's `vips fastcor` / `vips spcor`."""
    a, b, o = (str(tmp_path / n) for n in ("in.v", "ref.v", "out.v"))
    helpers.write_v(a, im, interp)
    helpers.write_v(b, ref, MULTIBAND)
    run_vips([op, a, b, o])
    return helpers.read_v(o)


def common_dtype(a, b):
    """vips__formatalike of two non-complex formats (arithmetic.c:76-109), for the kernel's name."""
    a, b = np.dtype(a), np.dtype(b)
    if a == b:
        return a
    if np.float64 in (a, b):
        return np.dtype(np.float64)
    if np.float32 in (a, b):
        return np.dtype(np.float32)
    signed = a.kind == "i" or b.kind == "i"
    size = max(a.itemsize, b.itemsize)
    if signed and any(d.kind == "u" and d.itemsize == size for d in (a, b)):
        size = min(4, size * 2)
    return np.dtype("%s%d" % ("i" if signed else "u", size))


def check(tmp_path, op, im, ref, what, interp=MULTIBAND):
    """One correlation on the device against the reference: bytes, header, the kernel that ran and its launches."""
    want, want_interp = ref_cor(tmp_path, op, im, ref, interp)
    with gated() as g:
        out = getattr(Image.new_from_array(im, interp), op)(Image.new_from_array(ref))
        got, got_interp = out.numpy(), lib.vips_hip_image_get_interpretation(out._h)
    what = "%s %s: %s %s against %s %s" % (what, op, im.shape, im.dtype, ref.shape, ref.dtype)
    same(got, want, what)
    assert got_interp == want_interp, (what, got_interp, want_interp)
    assert g.ran == {op + "_" + SUFFIX[common_dtype(im.dtype, ref.dtype)]: 1}, (what, g.ran)
    if im.dtype == ref.dtype:
        assert g.others == {}, (what, g.others)
    else:
        assert 1 <= sum(g.others.values()) <= 2, (what, g.others)
    return got


_cache = {}


def noise(w, h, bands, dtype=np.uint8, seed=5):
    """Seeded noise over the format's range (int: +- 2^30; float and double: +- 300 with fractions), made once, never
    changed."""
    key = (w, h, bands, np.dtype(dtype), seed)
    if key not in _cache:
        rng = np.random.default_rng(seed)
        dt = np.dtype(dtype)
        if dt == np.int32:
            a = rng.integers(-2 ** 30, 2 ** 30, (h, w, bands), dtype=dt, endpoint=True)
        elif dt.kind in "ui":
            info = np.iinfo(dt)
            a = rng.integers(info.min, info.max, (h, w, bands), dtype=dt, endpoint=True)
        else:
            a = ((rng.random((h, w, bands)) - 0.5) * 600.0).astype(dt)
        a.setflags(write=False)
        _cache[key] = a
    return _cache[key]


# ---------------------------------------------------------------- every format

@pytest.mark.parametrize("ref_size", [(5, 4), (8, 7)], ids=["5x4", "8x7"])
@pytest.mark.parametrize("bands", [1, 3])
@pytest.mark.parametrize("dtype", DTYPES, ids=name_of)
@pytest.mark.parametrize("op", OPS)
def test_formats(tmp_path, op, dtype, bands, ref_size):
    """Odd and even ref sizes in both directions (an even ref is not centred), rows that are no multiple of 4 bytes."""
    check(tmp_path, op, noise(W, H, bands, dtype, 11), noise(ref_size[0], ref_size[1], bands, dtype, 13), "formats",
          interp=SRGB if bands == 3 else B_W)


@pytest.mark.parametrize("dtype,bands", [(np.uint8, 1), (np.uint16, 3), (np.float32, 2)], ids=["uchar", "ushort3", "float2"])
@pytest.mark.parametrize("op", OPS)
def test_tile_seams(tmp_path, op, dtype, bands):
    """An image one pel wider and one row taller than a block's tile with a ref one smaller than a tile edge: the seams
    and the halos of four blocks lie inside the image."""
    tw, th = lib.vips_hip_correlation_step(0), lib.vips_hip_correlation_step(1)
    check(tmp_path, op, noise(tw + 1, th + 1, bands, dtype, 17), noise(tw - 1, th - 1, bands, dtype, 19), "seams")


@pytest.mark.parametrize("sizes", [((W, H), (1, 1)), ((5, 4), (8, 7)), ((1, 1), (5, 4)), ((1, 1), (1, 1))],
                         ids=["ref1x1", "ref_larger", "image1x1", "both1x1"])
@pytest.mark.parametrize("dtype", [np.uint8, np.float32], ids=name_of)
@pytest.mark.parametrize("op", OPS)
def test_small(tmp_path, op, dtype, sizes):
    (w, h), (rw, rh) = sizes
    check(tmp_path, op, noise(w, h, 2, dtype, 23), noise(rw, rh, 2, dtype, 29), "small")


@pytest.mark.parametrize("dtype,bands", [(np.uint8, 1), (np.float64, 4)], ids=["uchar", "double4"])
@pytest.mark.parametrize("op", OPS)
def test_largest_ref(tmp_path, op, dtype, bands):
    """The largest ref the kernels take, in the smallest and in the largest element the LDS tile holds."""
    side = lib.vips_hip_correlation_step(2)
    assert side >= 64
    check(tmp_path, op, noise(9, 7, bands, dtype, 31), noise(side, side, bands, dtype, 37), "largest ref")


@pytest.mark.parametrize("op", OPS)
def test_ref_beyond_the_limit_refused(op):
    side = lib.vips_hip_correlation_step(2)
    im = Image.new_from_array(noise(9, 7, 1, np.uint8, 31))
    for rw, rh in ((side + 1, side), (side, side + 1)):
        with pytest.raises(VipsHipError, match=r"%s: .*refs up to %d x %d" % (op, side, side)):
            getattr(im, op)(Image.new_from_array(noise(rw, rh, 1, np.uint8, 41)))


# ---------------------------------------------------------------- matching

@pytest.mark.parametrize("order", ["image1_ref3", "image3_ref1"])
@pytest.mark.parametrize("dtype", [np.uint8, np.float32], ids=name_of)
@pytest.mark.parametrize("op", OPS)
def test_band_matching(tmp_path, op, dtype, order):
    """One band against three, both ways round.  A one-band ref against three bands is replicated: spcor's vips_linear
    then takes its single-constant loop with three bands.  A one-band image banded up takes the ref's interpretation
    (vips__bandup), as the reference's header shows."""
    ib, rb = (1, 3) if order == "image1_ref3" else (3, 1)
    check(tmp_path, op, noise(W, H, ib, dtype, 43), noise(8, 7, rb, dtype, 47), order, interp=SRGB if ib == 3 else B_W)


@pytest.mark.parametrize("op", OPS)
def test_bands_refused(op):
    with pytest.raises(VipsHipError, match="%s: not one band or 4 bands" % op):
        getattr(Image.new_from_array(noise(W, H, 3, np.uint8, 43)), op)(Image.new_from_array(noise(5, 4, 4, np.uint8, 47)))
    with pytest.raises(VipsHipError, match="%s: not one band or 4 bands" % op):
        getattr(Image.new_from_array(noise(W, H, 4, np.uint8, 43)), op)(Image.new_from_array(noise(5, 4, 3, np.uint8, 47)))


@pytest.mark.parametrize("pair", [(np.uint8, np.uint16), (np.int16, np.uint8), (np.uint8, np.float32)],
                         ids=["uchar_ushort", "short_uchar", "uchar_float"])
@pytest.mark.parametrize("op", OPS)
def test_format_matching(tmp_path, op, pair):
    check(tmp_path, op, noise(W, H, 3, pair[0], 53), noise(5, 4, 3, pair[1], 59), "formats matched")


# ---------------------------------------------------------------- spcor's special cases

@pytest.mark.parametrize("dtype", [np.uint8, np.float32, np.float64], ids=name_of)
def test_spcor_constant_ref(tmp_path, dtype):
    """c1 is zero: every element is +0.0, not NaN and not -0.0."""
    ref = np.full((4, 5, 2), 77, dtype)
    got = check(tmp_path, "spcor", noise(W, H, 2, dtype, 61), ref, "constant ref")
    assert not got.view(np.uint32).any()


@pytest.mark.parametrize("dtype", [np.uint8, np.float32], ids=name_of)
def test_spcor_constant_area(tmp_path, dtype):
    """Windows inside a flat area have sum2 == 0: +0.0 there and not NaN; a flat corner reaches the copied edge."""
    im = noise(W, H, 1, dtype, 67).copy()
    im[10:24, 12:30] = 9
    im[:6, :7] = 200 if np.dtype(dtype).kind == "u" else -100.5
    got = check(tmp_path, "spcor", im, noise(5, 4, 1, dtype, 71), "constant area")
    # window (x, y) covers image pels x - 2 .. x + 2, y - 2 .. y + 1
    assert not got[12:23, 14:28].view(np.uint32).any()
    assert not got[0:5, 0:5].view(np.uint32).any()
    assert not np.isnan(got).any()


@pytest.mark.parametrize("means", ["equal", "differing"])
@pytest.mark.parametrize("dtype", [np.uint8, np.int32, np.float32, np.float64], ids=name_of)
def test_spcor_linear_paths(tmp_path, dtype, means):
    """A three-band ref whose band means are equal takes vips_linear's single-constant loop (-rmean rounded to float
    first, float arithmetic); one whose means differ the vector loop (double arithmetic, rounded to float)."""
    ref = noise(8, 7, 3, dtype, 73).copy()
    if means == "equal":
        # the bands hold the same values in other places: integer sums are exact, and these float sums too
        if np.dtype(dtype).kind == "f":
            ref = np.round(ref)
        ref[:, :, 1] = ref[::-1, ::-1, 0]
        ref[:, :, 2] = np.roll(ref[:, :, 0], 3, axis=1)
        sums = [float(np.sum(ref[:, :, b].astype(np.float64))) for b in range(3)]
        assert sums[0] == sums[1] == sums[2]
    check(tmp_path, "spcor", noise(W, H, 3, dtype, 79), ref, means + " means")


# ---------------------------------------------------------------- fastcor's special cases

def test_fastcor_subnormal_squares(tmp_path):
    """Values around 1e-20: dif * dif is subnormal, and a kernel that flushes subnormals would write zeros."""
    im = (noise(W, H, 1, np.float32, 83) * np.float32(1e-22)).astype(np.float32)
    ref = (noise(5, 4, 1, np.float32, 89) * np.float32(1e-22)).astype(np.float32)
    tiny = float(np.finfo(np.float32).tiny)
    assert (float(np.abs(im).max()) + float(np.abs(ref).max())) ** 2 < tiny  # every product is subnormal
    got = check(tmp_path, "fastcor", im, ref, "subnormal")
    assert np.count_nonzero(got) == got.size and float(got.min()) < tiny


@pytest.mark.parametrize("dtype", [np.uint16, np.uint32], ids=name_of)
def test_fastcor_wraps(tmp_path, dtype):
    """Full-range input: the sum passes 2^32 within two taps, and the wrapped value is the answer."""
    im, ref = noise(W, H, 1, dtype, 97), noise(8, 7, 1, dtype, 101)
    got = check(tmp_path, "fastcor", im, ref, "wrap")
    # the unwrapped sum of the window at the centre pel, in Python integers
    x, y = W // 2, H // 2
    win = im[y - 3:y + 4, x - 4:x + 4, 0]
    exact = sum((int(r) - int(p)) ** 2 for r, p in zip(ref[:, :, 0].ravel(), win.ravel()))
    assert exact >= 2 ** 32 and int(got[y, x, 0]) == exact % 2 ** 32


# ---------------------------------------------------------------- refusals

@pytest.mark.parametrize("op", OPS)
def test_refusals(op):
    real = Image.new_from_array(noise(W, H, 1, np.float32, 103))
    small = Image.new_from_array(noise(5, 4, 1, np.float32, 107))
    cplx = Image.new_from_array(np.zeros((4, 5, 1), np.complex64))
    with pytest.raises(VipsHipError, match="%s: image must be non-complex" % op):
        getattr(real, op)(cplx)
    with pytest.raises(VipsHipError, match="%s: image must be non-complex" % op):
        getattr(cplx, op)(small)
    fn = getattr(lib, "vips_hip_" + op)
    out = ctypes.c_void_p()
    for args in ((None, small._h, ctypes.byref(out)), (real._h, None, ctypes.byref(out)), (real._h, small._h, None)):
        assert fn(*args) == -1
        assert ("%s: null argument" % op) in _ffi.error_buffer()
        lib.vips_hip_error_clear()
    with pytest.raises(TypeError):
        getattr(real, op)(np.zeros((4, 5, 1), np.float32))


# ---------------------------------------------------------------- min / max of uint and int

def ref_extreme(tmp_path, op, a):
    path = str(tmp_path / "m.v")
    helpers.write_v(path, a, MULTIBAND)
    return float(run_vips([op, path]))


def check_extremes(tmp_path, a, what):
    im = Image.new_from_array(a)
    flat = a.reshape(a.shape[0] * a.shape[1], -1)
    for op, pick, arg in (("min", flat.min(axis=1), np.argmin), ("max", flat.max(axis=1), np.argmax)):
        with gated() as g:
            value, where = getattr(im, op)(with_options=True)
        assert sum(g.others.values()) == 1 and all(k.startswith("stats_") for k in g.others), (what, g.others)
        assert value == ref_extreme(tmp_path, op, a), (what, op, value)
        assert value == float(a.min() if op == "min" else a.max())
        first = int(arg(pick))  # numpy's first occurrence, in raster order
        assert (where["x"], where["y"]) == (first % a.shape[1], first // a.shape[1]), (what, op, where, first)
        assert getattr(im, op)() == value


@pytest.mark.parametrize("bands", [1, 3])
@pytest.mark.parametrize("dtype", [np.uint32, np.int32], ids=name_of)
def test_extremes_of_wide_integers(tmp_path, dtype, bands):
    """Noise: a unique extreme; with it written twice more in its band: a tie, the first in raster order wins."""
    a = noise(W, H, bands, dtype, 109).copy()
    info = np.iinfo(dtype)
    a[a == info.max] = info.max - 1
    a[a == info.min] = info.min + 1
    a[20, 30, bands - 1] = info.max
    a[21, 3, 0] = info.min
    check_extremes(tmp_path, a, "unique")
    a[20, 41, bands - 1] = a[33, 2, bands - 1] = info.max
    a[21, 50, 0] = a[36, 52, 0] = info.min
    check_extremes(tmp_path, a, "tie")


@pytest.mark.parametrize("place", ["first", "last"])
@pytest.mark.parametrize("dtype", [np.uint32, np.int32], ids=name_of)
def test_extremes_at_the_ends(tmp_path, dtype, place):
    """Both extremes at the first pel, or at the last; uint values above 2^31 compare as unsigned."""
    a = noise(W, H, 2, dtype, 113).copy()
    if dtype == np.uint32:
        a = a // 4 * 3 + 2 ** 30  # 2^30 .. 2^30 + 3 * 2^30: both sides of 2^31
        lo, hi = 5, 2 ** 32 - 7
        assert a.min() < 2 ** 31 < a.max()
    else:
        a = a // 2
        lo, hi = -2 ** 31, 2 ** 31 - 1
    y, x = (0, 0) if place == "first" else (H - 1, W - 1)
    a[y, x, 0], a[y, x, 1] = lo, hi
    check_extremes(tmp_path, a, place)


def test_uint_above_2_31_is_the_largest(tmp_path):
    a = np.full((4, 5, 1), 7, np.uint32)
    a[2, 3, 0] = 2 ** 31 + 5
    a[1, 1, 0] = 2 ** 31 - 1
    check_extremes(tmp_path, a, "above 2^31")
    value, where = Image.new_from_array(a).max(with_options=True)
    assert value == 2.0 ** 31 + 5 and (where["x"], where["y"]) == (3, 2)


def test_stats_still_refuse_wide_integers():
    for dtype in (np.uint32, np.int32):
        im = Image.new_from_array(noise(5, 4, 1, dtype, 127))
        for call in (im.stats, im.avg, im.deviate):
            with pytest.raises(VipsHipError, match="uint, int and double images are outside the HIP path"):
                call()
    with pytest.raises(VipsHipError, match="double images are outside the HIP path"):
        Image.new_from_array(noise(5, 4, 1, np.float64, 127)).min()


# ---------------------------------------------------------------- end to end

@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float32], ids=name_of)
def test_patch_is_found(dtype):
    """A patch cut from an image is found at its place, shifted by ref.size / 2 as the embed puts it."""
    im = noise(W, H, 1, dtype, 131)
    left, top, rw, rh = 17, 9, 8, 7
    patch = np.ascontiguousarray(im[top:top + rh, left:left + rw])
    dev, ref = Image.new_from_array(im), Image.new_from_array(patch)
    want = {"x": left + rw // 2, "y": top + rh // 2}
    value, where = dev.fastcor(ref).min(with_options=True)
    assert value == 0.0 and where == want, (value, where)
    value, where = dev.spcor(ref).max(with_options=True)
    assert abs(value - 1.0) < 1e-6 and where == want, (value, where)
