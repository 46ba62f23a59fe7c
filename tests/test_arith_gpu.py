"""GPU parity: arithmetic on the device -- vips_linear, vips_invert, vips_abs, vips_add, vips_subtract, vips_multiply,
vips_divide, vips_stats, vips_avg, vips_deviate, vips_min and vips_max (libvips_amd/csrc/arith.hip, ops_arith.cpp).

Everything is np.array_equal against the compiled reference -- values, dtype, shape and, for two images, the result's
header -- unless a test says otherwise: the pointwise operations are the reference's expressions with separate
multiplies and adds and a correctly rounded division, integer statistics are exact, and the float statistics are
compared on images whose sums are exact in any order (integer-valued pels) or against math.fsum within the bound of
any double summation order.  One-image operations and vips_stats reach the reference through Ref.run, two-image
operations through its command line.  The streaming and the one-element-a-lane kernel are swept over element sizes,
band counts, row lengths round the streaming kernel's groups and a block of them, on windows of larger frames, against
numpy models that the whole-domain tests pin to the reference; every sweep case asserts by the gate report which
kernel ran and that it was launched once.
NaN is kept out of the pointwise inputs: which NaN an operation makes of a NaN (sign, payload) is the processor's
choice, not the reference's.  Runs on the CPU too, on host fibers (tests/test_emul_arith.py)."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import libvips_amd
from libvips_amd import Image, VipsHipError, _ffi
from tests import helpers
from tests.helpers import Ref

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not helpers.have_ref(), reason="oracle/_ref not built")]

lib = _ffi.lib
INTERP = helpers.INTERP
VIPS = os.path.join(helpers.ROOT, "oracle", "_ref", "bin", "vips")
SENTINEL = 0xA5
ALL_DTYPES = [np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32, np.float32, np.float64]


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
                self.ran = {k: n for k, (n, _) in libvips_amd.gate_report().items() if k.startswith(("arith_", "stats_"))}
        finally:
            lib.vips_hip_gate_enable(0)
            lib.vips_hip_gate_reset()
        return False


class general_kernel(object):
    """The one-element-a-lane kernels for everything inside (the library reads the variable at every dispatch)."""

    def __init__(self, on=True):
        self.on = on

    def __enter__(self):
        if self.on:
            os.environ["VIPS_HIP_NO_ARITH_STREAM"] = "1"

    def __exit__(self, *exc):
        os.environ.pop("VIPS_HIP_NO_ARITH_STREAM", None)
        return False


def same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), what


def extremes_of(dtype):
    dtype = np.dtype(dtype)
    if dtype.kind in "ui":
        info = np.iinfo(dtype)
        return np.array([info.min, info.min + 1, -1 if info.min < 0 else 1, 0, 1, info.max - 1, info.max], dtype)
    info = np.finfo(dtype)
    # the largest and the smallest normal numbers, a subnormal, both zeros and both infinities
    return np.array([info.max, -info.max, info.tiny, -info.tiny, info.tiny / 4, 0.0, -0.0, np.inf, -np.inf, 1.0, -1.5, 255.5,
                     16777217.0, 0.1], dtype)


def noise(w, h, dtype, bands, seed, with_extremes=False, finite=False):
    """Seeded noise over the format's range (floats: +- 300 with fractions), the format's extremes first (finite: less
    the infinities, for operands that would make NaN of them: inf - inf, 0 * inf)."""
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(seed)
    n = w * h * bands
    if dtype.kind in "ui":
        info = np.iinfo(dtype)
        a = rng.integers(info.min, info.max, n, dtype=dtype, endpoint=True)
    else:
        a = ((rng.random(n) - 0.5) * 600.0).astype(dtype)
    if with_extremes:
        ext = extremes_of(dtype)
        if finite and dtype.kind == "f":
            ext = ext[np.isfinite(ext)]
        a[:len(ext)] = ext
    return np.ascontiguousarray(a.reshape(h, w, bands))


def vec(v):
    return " ".join(repr(float(x)) for x in np.atleast_1d(v))


def ref_linear(src, a, b, uchar=False, interp=0):
    args = "a=%s,b=%s%s" % (vec(a), vec(b), ",uchar=true" if uchar else "")
    return Ref.run_interp("linear", src, args, interpretation=interp)


def dev_linear(src, a, b, uchar=False, interp=0):
    out = Image.new_from_array(src, interp).linear(a, b, uchar=uchar)
    return out.numpy(), lib.vips_hip_image_get_interpretation(out._h)


def check_linear(src, a, b, uchar, what, interp=0, kernel=None):
    want, want_interp = ref_linear(src, a, b, uchar, interp)
    with gated() as g:
        got, got_interp = dev_linear(src, a, b, uchar, interp)
    same(got, want, what)
    # (the shim reads an interpretation of 0 as "derive one from the bands and the format": nothing to compare then)
    assert interp == 0 or got_interp == want_interp, (what, got_interp, want_interp)
    assert sum(g.ran.values()) == 1 and (kernel is None or g.ran == {kernel: 1}), (what, g.ran)


# the constants of the whole-domain tests: a fraction that is inexact in float (the separate multiply and add),
# products below 0 and above 255 (the uchar clip), a band vector with two equal elements and one different
SINGLE = [(1.1, -20.3), (-1.5, 300.0), ([0.25, 0.25, 0.25], [7.0])]
VECTORS = {3: [([1.1, 1.1, -2.5], [-20.3, 7.25, 300.0]), ([1.1], [0.0, 0.0, 0.5]), ([1.1, 1.1, 3.0], [-20.3])],
           4: [([1.1, 1.1, -2.5, 0.3], [-20.3, 7.25, 300.0, 7.25])]}


# ---------------------------------------------------------------- linear: whole domains, every arithmetic shape

@pytest.mark.parametrize("uchar", [False, True], ids=["float", "uchar"])
@pytest.mark.parametrize("bands", [1, 3, 4])
def test_linear_every_uchar(bands, uchar):
    """All 256 values in every band: LOOP1 / LOOP1uc with one constant, LOOPN / LOOPNuc with band vectors (a one-band
    image against a three-vector makes three bands)."""
    src = np.empty((1, 256, bands), np.uint8)
    for k in range(bands):
        src[0, :, k] = (np.arange(256) + 37 * k) & 255
    for a, b in SINGLE:
        if bands == 4 and len(np.atleast_1d(a)) == 3:
            continue
        check_linear(src, a, b, uchar, ("single", bands, a, b, uchar))
    for a, b in VECTORS[3 if bands == 1 else bands]:
        check_linear(src, a, b, uchar, ("vector", bands, a, b, uchar), interp=INTERP["b-w"] if bands == 1 else INTERP["srgb"])


@pytest.mark.parametrize("uchar", [False, True], ids=["float", "uchar"])
def test_linear_every_ushort(uchar):
    src = np.arange(65536, dtype=np.uint16).reshape(256, 256, 1)
    for a, b in [(1.1, -20.3), (0.004, -5.3), (-0.001, 30.7)]:
        check_linear(src, a, b, uchar, ("single", a, b, uchar), kernel="arith_stream")
    # one band against a three-vector: the general kernel, the input indexed by pel
    for a, b in [([0.004, 0.004, -0.01], [-5.3, 7.25, 300.0]), ([1.1, 1.1, -2.5], [-20.3])]:
        check_linear(src, a, b, uchar, ("vector", a, b, uchar), kernel="arith_general")


@pytest.mark.parametrize("uchar", [False, True], ids=["float", "uchar"])
@pytest.mark.parametrize("dtype", [np.int8, np.int16, np.uint32, np.int32, np.float32, np.float64], ids=lambda d: np.dtype(d).name)
def test_linear_formats(dtype, uchar):
    """Seeded noise and the format's extremes, 64 x 33 x 3, the four arithmetic shapes."""
    src = noise(64, 33, dtype, 3, 11, with_extremes=True)
    for a, b in SINGLE[:2] + VECTORS[3][:1]:
        check_linear(src, a, b, uchar, (np.dtype(dtype).name, a, b, uchar), interp=INTERP["srgb"], kernel="arith_stream")
    one = np.ascontiguousarray(src[:, :, :1])
    check_linear(one, [1.1, 1.1, -2.5], [-20.3, 7.25, 300.0], uchar, (np.dtype(dtype).name, "one band against three"),
                 kernel="arith_general")


def test_linear_errors_and_operators():
    src = noise(9, 7, np.uint8, 3, 13)
    im = Image.new_from_array(src, "srgb")
    with pytest.raises(RuntimeError) as ref:
        Ref.run("linear", src, "a=1 2,b=0")
    with pytest.raises(VipsHipError) as dev:
        im.linear([1, 2], 0)
    assert str(ref.value).strip().split(": ")[-1] in str(dev.value)
    z = (noise(5, 4, np.float32, 1, 15) + 1j * noise(5, 4, np.float32, 1, 17)).astype(np.complex64)
    for fn in (lambda i: i.linear(1, 2), lambda i: i.invert(), lambda i: i.abs(), lambda i: i.add(i), lambda i: i.stats()):
        with pytest.raises(VipsHipError, match="image must be non-complex"):
            fn(Image.new_from_array(z))
    same((im * 1.1 + [-20.3, 7.25, 300.0]).numpy(), Ref.run("linear", Ref.run("linear", src, "a=1.1,b=0"), "a=1,b=-20.3 7.25 300"), "* +")
    same((2 - im).numpy(), Ref.run("linear", src, "a=-1,b=2"), "rsub")
    same((im - [1, 2, 3]).numpy(), Ref.run("linear", src, "a=1,b=-1 -2 -3"), "sub")
    same((im / 4).numpy(), Ref.run("linear", src, "a=0.25,b=0"), "div")
    same((-im).numpy(), Ref.run("linear", src, "a=-1,b=0"), "neg")
    other = Image.new_from_array(noise(9, 7, np.uint8, 3, 19), "srgb")
    same((im + other).numpy(), im.add(other).numpy(), "+")
    same((im - other).numpy(), im.subtract(other).numpy(), "-")
    same((im * other).numpy(), im.multiply(other).numpy(), "*")
    same((im / other).numpy(), im.divide(other).numpy(), "/")


# ---------------------------------------------------------------- invert, abs

def every_value(dtype):
    info = np.iinfo(dtype)
    a = np.arange(info.min, info.max + 1, dtype=np.int64).astype(dtype)
    return a.reshape((1, 256, 1) if a.size == 256 else (256, 256, 1))


@pytest.mark.parametrize("nick", ["invert", "abs"])
@pytest.mark.parametrize("dtype", ALL_DTYPES, ids=lambda d: np.dtype(d).name)
def test_invert_abs(nick, dtype):
    """Every value of the 8- and 16-bit formats; noise and the extremes (INT_MIN among them) of the others."""
    src = every_value(dtype) if np.dtype(dtype).itemsize < 4 else noise(64, 33, dtype, 3, 21, with_extremes=True)
    want, want_interp = Ref.run_interp(nick, src, "", interpretation=INTERP["b-w"])
    with gated() as g:
        out = getattr(Image.new_from_array(src, "b-w"), nick)()
        got = out.numpy()
    same(got, want, (nick, np.dtype(dtype).name))
    assert lib.vips_hip_image_get_interpretation(out._h) == want_interp
    copies = nick == "abs" and np.dtype(dtype).kind == "u"  # abs.c:88-90
    assert g.ran == ({} if copies else {"arith_stream": 1}), g.ran


def test_invert_anchor():
    """What the reference was seen to make of char -1, -28, 34."""
    a = np.array([-1, -28, 34], np.int8).reshape(1, 3, 1)
    assert Image.new_from_array(a).invert().numpy().ravel().tolist() == [1, 28, -34]
    assert Ref.run("invert", a).ravel().tolist() == [1, 28, -34]


# ---------------------------------------------------------------- both kernels over geometries, on windows of frames

def model_invert(src):
    if src.dtype.kind == "u":
        return np.iinfo(src.dtype).max - src
    return -src


def model_linear(src, a, b, uchar):
    """LOOPN / LOOPNuc in numpy (no fused multiply-add there); pinned to the reference by the tests above and below."""
    k = np.arange(src.shape[2])
    a, b = np.asarray(a, np.float64)[k], np.asarray(b, np.float64)[k]
    if uchar:
        t = a * src.astype(np.float64) + b
        return np.trunc(np.clip(t, 0, 255)).astype(np.uint8)
    if src.dtype == np.float64:
        return a * src + b
    return (a * src.astype(np.float32).astype(np.float64) + b).astype(np.float32)


def model_linear_single(src, a, b, uchar):
    """LOOP1 / LOOP1uc for integer and float images: float constants, float multiply, float add."""
    t = np.float32(a) * src.astype(np.float32) + np.float32(b)
    return np.trunc(np.clip(t, 0, 255)).astype(np.uint8) if uchar else t


def upload_frame(frame):
    return Image.new_from_array(np.ascontiguousarray(frame)[:, :, None])


def gen_in_frames(src, out_dtype, out_bands, call, margin, odd_stride=False):
    """A generate function with the input and the output as windows of larger frames: `margin` bytes before a row's
    first pel (0 or 4: rows start on dwords; 1 .. 3: they need not), strides that are multiples of 4 (margin 0, 4) or
    odd.  odd_stride (elements of 1 or 2 bytes): strides one element past a multiple of 4, the margins such that the
    window's first row still starts on a dword.  The output frame's bytes outside the window must stay as they were."""
    h, w, b = src.shape
    ipel, opel = b * src.dtype.itemsize, out_bands * np.dtype(out_dtype).itemsize
    # rows must start on whole elements: aligned frames keep doubles on 8 bytes, unaligned ones move a row's start by
    # one element
    ies, oes = src.dtype.itemsize, np.dtype(out_dtype).itemsize
    imargin, iunit = (max(4, ies), max(4, ies)) if margin % 4 == 0 else (margin * ies, ies)
    omargin, ounit = (max(4, oes), max(4, oes)) if margin % 4 == 0 else (margin * oes, oes)
    istride = (imargin + w * ipel + 5 + iunit - 1) // iunit * iunit
    ostride = (omargin + w * opel + 7 + ounit - 1) // ounit * ounit
    if odd_stride:
        assert margin % 4 == 0 and ies < 4 and oes < 4
        istride, ostride = istride + 4 + ies, ostride + 4 + oes
        # (the window is on row 1 of a frame that starts on a dword)
        imargin, omargin = 4 + -istride % 4, 4 + -ostride % 4
    fin = np.full((h + 2, istride), 0x3C, np.uint8)
    fin[1:1 + h, imargin:imargin + w * ipel] = src.view(np.uint8).reshape(h, w * ipel)
    fout = np.full((h + 2, ostride), SENTINEL, np.uint8)
    din, dout = upload_frame(fin), upload_frame(fout)
    rin = _ffi.Region(din.data_ptr + istride + imargin, 3, 1, w, h, w + 9, h + 5, b, helpers.DTYPE_FORMATS[src.dtype], istride)
    rout = _ffi.Region(dout.data_ptr + ostride + omargin, 3, 1, w, h, w + 9, h + 5, out_bands,
                       helpers.DTYPE_FORMATS[np.dtype(out_dtype)], ostride)
    _ffi.check(call(ctypes.byref(rin), ctypes.byref(rout)))
    back = dout.numpy()[:, :, 0]
    got = back[1:1 + h, omargin:omargin + w * opel].copy()
    back[1:1 + h, omargin:omargin + w * opel] = SENTINEL
    assert (back == SENTINEL).all(), "bytes outside the output window were written"
    return np.ascontiguousarray(got).view(out_dtype).reshape(h, w, out_bands)


def sweep_widths(pel, out_es):
    """Widths whose rows are 1, 15, 16, 17, 47, 48, 49 bytes (rounded up to whole pels) and one block's worth of the
    streaming kernel's groups - 1 / + 0 / + 1 pel."""
    block = lib.vips_hip_arith_step(0) * lib.vips_hip_arith_step(1) // out_es  # elements of the output a block makes
    bands = pel // out_es if pel % out_es == 0 else 1
    return sorted({-(-n // pel) for n in (1, 15, 16, 17, 47, 48, 49)} | {max(1, block // bands + d) for d in (-1, 0, 1)})


SWEEP_DTYPES = {1: np.uint8, 2: np.uint16, 4: np.float32, 8: np.float64}


@pytest.mark.parametrize("kernel", ["stream", "general", "unaligned"])
@pytest.mark.parametrize("bands", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("es", [1, 2, 4, 8])
def test_invert_sweep(es, bands, kernel):
    """stream: rows on dwords; general: the same under VIPS_HIP_NO_ARITH_STREAM; unaligned: rows that start one
    element off a dword wherever the element is smaller than one, which the stream declines."""
    dtype = SWEEP_DTYPES[es]
    for w in sweep_widths(es * bands, es):
        for h in (2, 33):
            src = noise(w, h, dtype, bands, 1000 + w)
            margin = 1 if kernel == "unaligned" else 4
            with general_kernel(kernel == "general"), gated() as g:
                got = gen_in_frames(src, dtype, bands, lib.vips_hip_invert_gen, margin)
            streams = kernel == "stream" or (kernel == "unaligned" and es >= 4)
            assert g.ran == {"arith_stream" if streams else "arith_general": 1}, (g.ran, es, bands, w, h)
            same(got, model_invert(src), (kernel, es, bands, w, h))


@pytest.mark.parametrize("kernel", ["stream", "general"])
@pytest.mark.parametrize("bands", [1, 3])
@pytest.mark.parametrize("es", [1, 2])
def test_invert_one_row_sweep(es, bands, kernel):
    """One row is nothing away from a next one, so its stride has no say: a one-row window that starts on a dword
    streams out of frames whose strides are no multiple of 4; the general kernel gives the same bytes."""
    dtype = SWEEP_DTYPES[es]
    for w in sweep_widths(es * bands, es):
        src = noise(w, 1, dtype, bands, 3000 + w)
        with general_kernel(kernel == "general"), gated() as g:
            got = gen_in_frames(src, dtype, bands, lib.vips_hip_invert_gen, 4, odd_stride=True)
        assert g.ran == {"arith_stream" if kernel == "stream" else "arith_general": 1}, (g.ran, es, bands, w)
        same(got, model_invert(src), (kernel, es, bands, w))


@pytest.mark.parametrize("kernel", ["stream", "general"])
@pytest.mark.parametrize("uchar", [False, True], ids=["float", "uchar"])
@pytest.mark.parametrize("bands", [1, 2, 3, 4, 5])
def test_linear_vector_sweep(bands, uchar, kernel):
    """The band vector of a group: constants picked by (element index) mod bands, over every group phase."""
    a = [1.1, 1.1, -2.5, 0.3, 7.0][:bands] if bands > 1 else [1.1, 1.1, -2.5]
    b = [-20.3, 7.25, 300.0, 7.25, -9.5][:bands] if bands > 1 else [-20.3, 7.25, 300.0]
    out_bands = bands if bands > 1 else 3
    args = Image.linear_args(a, b, uchar)
    for dtype in (np.uint8, np.uint16, np.float32, np.float64):
        out_dtype = np.uint8 if uchar else (np.float64 if dtype == np.float64 else np.float32)
        for w in sweep_widths(np.dtype(out_dtype).itemsize * out_bands, np.dtype(out_dtype).itemsize):
            for h in (2, 33):
                src = noise(w, h, dtype, bands, 2000 + w)
                with general_kernel(kernel == "general"), gated() as g:
                    got = gen_in_frames(src, out_dtype, out_bands,
                                        lambda i, o: lib.vips_hip_linear_gen(ctypes.byref(args), i, o), 4)
                streams = kernel == "stream" and bands > 1
                assert g.ran == {"arith_stream" if streams else "arith_general": 1}, (g.ran, bands, w, h)
                wide = src if bands > 1 else np.repeat(src, 3, axis=2)
                same(got, model_linear(wide, a, b, uchar), (kernel, np.dtype(dtype).name, bands, uchar, w, h))


def test_the_models_are_the_reference():
    for dtype in (np.uint8, np.uint16, np.float32, np.float64):
        src = noise(19, 5, dtype, 3, 31)
        same(model_invert(src), Ref.run("invert", src), ("invert", dtype))
        for uchar in (False, True):
            a, b = [1.1, 1.1, -2.5], [-20.3, 7.25, 300.0]
            same(model_linear(src, a, b, uchar), ref_linear(src, a, b, uchar)[0], ("linear", dtype, uchar))
            if dtype != np.float64:
                same(model_linear_single(src, 0.004, -5.3, uchar), ref_linear(src, 0.004, -5.3, uchar)[0], ("linear, one constant", dtype, uchar))


# ---------------------------------------------------------------- whole images: any width streams; the grid's stride

@pytest.mark.parametrize("shape", [(21, 9, 3, np.uint8), (1023, 3, 3, np.uint8), (33, 7, 1, np.uint16), (5, 3, 1, np.uint8)],
                         ids=lambda s: "%dx%dx%d-%s" % (s[0], s[1], s[2], np.dtype(s[3]).name))
def test_whole_images_stream_whatever_their_width(shape):
    """Rows of a whole image follow one another without a gap and are one row to the stream kernel: row bytes that are
    no multiple of 4 stream too."""
    w, h, bands, dtype = shape
    assert w * bands * np.dtype(dtype).itemsize % 4
    src, other = noise(w, h, dtype, bands, 401), noise(w, h, dtype, bands, 403)
    im, im2 = Image.new_from_array(src), Image.new_from_array(other)
    a, b = ([1.1, 1.1, -2.5], [-20.3, 7.25, 300.0]) if bands == 3 else (0.004, -5.3)
    model = model_linear if bands == 3 else model_linear_single
    wide = src.astype(np.int64)
    cases = [("invert", lambda: im.invert(), model_invert(src)),
             ("linear", lambda: im.linear(a, b), model(src, a, b, False)),
             ("linear uchar", lambda: im.linear(a, b, uchar=True), model(src, a, b, True)),
             ("add", lambda: im.add(im2), (wide + other).astype(np.uint16 if dtype == np.uint8 else np.uint32)),
             ("subtract", lambda: im.subtract(im2), (wide - other).astype(np.int16 if dtype == np.uint8 else np.int32))]
    for name, fn, want in cases:
        with gated() as g:
            got = fn().numpy()
        assert g.ran == {"arith_stream": 1}, (name, g.ran)
        same(got, want, (name, shape))


def over_the_grid(out_es, bands):
    """A square side whose image has a few more 16-byte groups of output than a capped grid takes in one step, the last
    group ragged."""
    elems = (lib.vips_hip_arith_step(2) * lib.vips_hip_arith_step(0) + 700) * (lib.vips_hip_arith_step(1) // out_es) + 3
    return int(math.isqrt(elems // bands)) + 1


def test_pointwise_grid_stride():
    """More groups than the capped grid has lanes: the lanes' second step, for one and for two operands and for band
    vectors, which must keep their phase across the step."""
    side = over_the_grid(1, 3)
    src, other = noise(side, side, np.uint8, 3, 411), noise(side, side, np.uint8, 3, 413)
    assert -(-side * side * 3 // 16) > lib.vips_hip_arith_step(2) * lib.vips_hip_arith_step(0)
    im, im2 = Image.new_from_array(src), Image.new_from_array(other)
    a, b = [1.1, 1.1, -2.5], [-20.3, 7.25, 300.0]
    for name, fn, want in (("invert", lambda: im.invert(), model_invert(src)),
                           ("linear uchar", lambda: im.linear(a, b, uchar=True), model_linear(src, a, b, True))):
        with gated() as g:
            got = fn().numpy()
        assert g.ran == {"arith_stream": 1}, (name, g.ran)
        same(got, want, name)
    side = over_the_grid(2, 1)
    src, other = noise(side, side, np.uint8, 1, 415), noise(side, side, np.uint8, 1, 417)
    with gated() as g:
        got = Image.new_from_array(src).multiply(Image.new_from_array(other)).numpy()
    assert g.ran == {"arith_stream": 1}, g.ran
    same(got, src.astype(np.uint16) * other, "multiply")


VECTOR_A, VECTOR_B = [1.1, 1.1, -2.5], [-20.3, 7.25, 300.0]


@pytest.mark.parametrize("case", ["invert", "linear-ushort-to-uchar", "linear-uchar-to-float"])
def test_second_turn_of_the_stream_in_frames(case):
    """Rows that stay rows: a window of a larger frame whose rows together have more 16-byte groups than the capped grid
    has lanes, so that a lane's second group is on another row, at another place of it and at another phase of the band
    vector; every row ends in a ragged group, and nothing outside the window is written."""
    dtype, out_dtype = {"invert": (np.uint8, np.uint8), "linear-ushort-to-uchar": (np.uint16, np.uint8),
                        "linear-uchar-to-float": (np.uint8, np.float32)}[case]
    lanes = lib.vips_hip_arith_step(2) * lib.vips_hip_arith_step(0)
    per_group = lib.vips_hip_arith_step(1) // np.dtype(out_dtype).itemsize
    width = (4096 // np.dtype(out_dtype).itemsize + 3 + 2) // 3
    groups = -(-width * 3 // per_group)
    height = lanes // groups + 9
    assert width * 3 % per_group and height > 1 and groups * height > lanes
    # the lane's second group is elsewhere in its row, at another phase of the three constants
    assert lanes % groups and lanes % groups * per_group % 3
    src = noise(width, height, dtype, 3, 421)
    if case == "invert":
        call, want = lib.vips_hip_invert_gen, model_invert(src)
    else:
        args = Image.linear_args(VECTOR_A, VECTOR_B, out_dtype == np.uint8)
        call, want = (lambda i, o: lib.vips_hip_linear_gen(ctypes.byref(args), i, o)), model_linear(src, VECTOR_A, VECTOR_B, out_dtype == np.uint8)
    with gated() as g:
        got = gen_in_frames(src, out_dtype, 3, call, 4)
    assert g.ran == {"arith_stream": 1}, g.ran
    same(got, want, case)


@pytest.mark.parametrize("case", [(1, 3, 3), (3, 2, 3), (3, 2, 1)], ids=lambda c: "%dblocks-%dbands" % (c[0], c[2]))
def test_second_turn_of_the_general_kernel(case):
    """The one-element-a-lane kernel with more rows than grid.y, which is the cap for rows of one block and a third of it
    for rows of three (the last ragged); one band against a three-vector reaches it without the switch."""
    blocks, extra, bands = case
    threads, cap = lib.vips_hip_arith_step(0), lib.vips_hip_arith_step(2)
    width = ((blocks - 1) * threads + 63) // 3
    in_flight = -(-cap // -(-width * 3 // threads))
    rows = in_flight + extra
    assert -(-width * 3 // threads) == blocks and rows > in_flight and (blocks == 1) == (in_flight == cap) and width * 3 % threads
    src = noise(width, rows, np.uint16, bands, 431)
    args = Image.linear_args(VECTOR_A, VECTOR_B, False)
    with general_kernel(bands == 3), gated() as g:
        got = gen_in_frames(src, np.float32, 3, lambda i, o: lib.vips_hip_linear_gen(ctypes.byref(args), i, o), 4)
    assert g.ran == {"arith_general": 1}, g.ran
    same(got, model_linear(src if bands == 3 else np.repeat(src, 3, axis=2), VECTOR_A, VECTOR_B, False), case)


# ---------------------------------------------------------------- two images: the reference's command line

OPS = ["add", "subtract", "multiply", "divide"]


def ref_cli(tmp_path, op, images):
    """-> (array, interpretation) of `vips <op> a.v b.v out.v`; RuntimeError with its words."""
    paths = []
    for i, (array, interp) in enumerate(images):
        paths.append(str(tmp_path / ("in%d.v" % i)))
        helpers.write_v(paths[-1], array, interp)
    out = str(tmp_path / "out.v")
    r = subprocess.run([VIPS, op] + paths + [out], env=helpers.ref_cli_env(), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True)
    if r.returncode != 0:
        raise RuntimeError(r.stderr.strip() or "vips %s failed" % op)
    return helpers.read_v(out)


def check_two(tmp_path, op, a, b, what, kernel=None):
    """The device's result and header against the reference's, or both an error with the reference's words."""
    (sa, ia), (sb, ib) = a, b
    da, db = Image.new_from_array(sa, ia), Image.new_from_array(sb, ib)
    try:
        want, want_interp = ref_cli(tmp_path, op, [a, b])
    except RuntimeError as e:
        words = str(e).strip().splitlines()[-1]
        with pytest.raises(VipsHipError) as info:
            getattr(da, op)(db)
        assert words.split(": ", 1)[-1] in str(info.value) and str(info.value).startswith(op + ":"), (what, words, str(info.value))
        return None
    with gated() as g:
        out = getattr(da, op)(db)
        got = out.numpy()
    assert (out.width, out.height, out.bands) == (want.shape[1], want.shape[0], want.shape[2]), (what, "size")
    same(got, want, (op, what))
    assert lib.vips_hip_image_get_interpretation(out._h) == want_interp, (op, what, "interpretation")
    # ONE launch, whatever had to be matched
    assert g.ran == {kernel: 1} if kernel else sum(g.ran.values()) == 1, (op, what, g.ran)
    return got


@pytest.mark.parametrize("kernel", ["stream", "general"])
@pytest.mark.parametrize("op", OPS)
def test_binary_every_uchar_pair(tmp_path, op, kernel):
    x, y = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8))
    a, b = (np.ascontiguousarray(x[:, :, None]), INTERP["b-w"]), (np.ascontiguousarray(y[:, :, None]), INTERP["b-w"])
    with general_kernel(kernel == "general"):
        check_two(tmp_path, op, a, b, "all pairs", kernel="arith_" + kernel)


@pytest.mark.parametrize("op", OPS)
def test_binary_float(tmp_path, op):
    """Noise with zeros (both signs) among the divisors, the extremes, and quotients that are inexact."""
    a = noise(64, 33, np.float32, 3, 41, with_extremes=True, finite=True)
    b = noise(64, 33, np.float32, 3, 43)
    b.ravel()[5::7] = 0.0
    b.ravel()[6::14] = -0.0
    b.ravel()[:16] = [3.0, 7.0, 0.1, 1e-30, 1e30, 3.0, 0.0, 2.0, 2.0, 49.0, -3.0, 1.1, 3.0, 10.0, 0.7, 1e-3]
    check_two(tmp_path, op, (a, INTERP["srgb"]), (b, INTERP["srgb"]), "float", kernel="arith_stream")
    one = np.arange(1, 64 * 33 * 3 + 1, dtype=np.float32).reshape(33, 64, 3)
    three = np.full_like(one, 3.0)
    check_two(tmp_path, op, (one, INTERP["srgb"]), (three, INTERP["srgb"]), "thirds")
    d = noise(17, 9, np.float64, 2, 45, with_extremes=True, finite=True)
    e = noise(17, 9, np.float64, 2, 47)
    e.ravel()[::5] = 0.0
    check_two(tmp_path, op, (d, 0), (e, 0), "double")


PAIRS = [(np.uint8, np.int8), (np.uint8, np.uint16), (np.uint16, np.int16), (np.uint32, np.int32), (np.uint8, np.float32),
         (np.float32, np.float64)]


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: "%s-%s" % (np.dtype(p[0]).name, np.dtype(p[1]).name))
def test_binary_format_pairs(tmp_path, op, pair):
    """vips__formatalike, both orders.  Products that overflow int are kept out (signed overflow is no contract)."""
    a, b = (noise(21, 9, t, 3, seed, with_extremes=True, finite=True) for t, seed in zip(pair, (51, 53)))
    if op == "multiply" and np.dtype(pair[0]).itemsize == 4 and np.dtype(pair[0]).kind != "f":
        a, b = (a % 40000).astype(pair[0]), (b % 40000 - 20000).astype(pair[1])
    b.ravel()[3::11] = 0
    check_two(tmp_path, op, (a, INTERP["srgb"]), (b, INTERP["srgb"]), "left, right")
    check_two(tmp_path, op, (b, INTERP["srgb"]), (a, INTERP["srgb"]), "right, left")


@pytest.mark.parametrize("op", OPS)
def test_binary_bands_and_sizes(tmp_path, op):
    """vips__bandalike: one band against three in both orders, three against four refused; vips__sizealike: 7 x 5
    against 4 x 9, both operands embedded -- every case one launch of the general kernel."""
    one, three = (noise(9, 7, np.uint8, 1, 61), INTERP["b-w"]), (noise(9, 7, np.uint8, 3, 63), INTERP["srgb"])
    four = (noise(9, 7, np.uint8, 4, 65), INTERP["srgb"])
    check_two(tmp_path, op, one, three, "1 against 3", kernel="arith_general")
    check_two(tmp_path, op, three, one, "3 against 1", kernel="arith_general")
    assert check_two(tmp_path, op, three, four, "3 against 4") is None
    assert check_two(tmp_path, op, four, three, "4 against 3") is None
    for dtype in (np.uint8, np.float32):
        a, b = (noise(7, 5, dtype, 3, 67), INTERP["srgb"]), (noise(4, 9, dtype, 3, 69), INTERP["srgb"])
        check_two(tmp_path, op, a, b, "7x5 against 4x9", kernel="arith_general")
        check_two(tmp_path, op, b, a, "4x9 against 7x5", kernel="arith_general")
    a, b = (noise(7, 5, np.int16, 1, 71), INTERP["b-w"]), (noise(4, 9, np.uint8, 3, 73), INTERP["srgb"])
    check_two(tmp_path, op, a, b, "7x5x1 short against 4x9x3 uchar")


@pytest.mark.parametrize("interps", [("srgb", "srgb"), ("b-w", "b-w"), ("multiband", "multiband"), ("b-w", "srgb"),
                                     ("srgb", "b-w"), ("multiband", "srgb"), ("srgb", "multiband")], ids="-".join)
def test_binary_headers(tmp_path, interps):
    """Size, bands, format and interpretation of the result are the reference's."""
    bands = {"srgb": 3, "b-w": 1, "multiband": 3}
    a = (noise(6, 4, np.uint8, bands[interps[0]], 81), INTERP[interps[0]])
    b = (noise(5, 5, np.uint16, bands[interps[1]], 83), INTERP[interps[1]])
    for op in OPS:
        check_two(tmp_path, op, a, b, interps)


# ---------------------------------------------------------------- stats

STATS_DTYPES = [np.uint8, np.int8, np.uint16, np.int16, np.float32]


def quiet(w, h, dtype, bands, seed):
    """Integer-valued noise well inside the format's range, so that extremes can be placed."""
    rng = np.random.default_rng(seed)
    lo, hi = (-90, 90) if np.dtype(dtype).kind in "if" else (20, 200)
    return rng.integers(lo, hi, (h, w, bands)).astype(dtype)


def place(a, pel_min, pel_max):
    """Unique extremes: band k's minimum at raster pel pel_min + k, its maximum at pel_max - k (distinct per band, so
    that row 0 has a unique winner too)."""
    h, w, bands = a.shape
    flat = a.reshape(h * w, bands)
    lo, hi = (-128, 127) if np.dtype(a.dtype).kind in "if" else (0, 255)
    for k in range(bands):
        flat[min(pel_min + k, h * w - 1), k] = lo + k
        flat[max(pel_max - k, 0), k] = hi - k
    return a


def check_stats(src, what, kernel=None, equal_nan=False):
    """equal_nan: the matrix is expected to hold NaN (a NaN among the pels; one pel, whose deviation is 0 / 0) and NaN
    counts as equal to NaN; otherwise the comparison is exact and a NaN on either side fails it."""
    want = Ref.run("stats", src)[:, :, 0]
    im = Image.new_from_array(src)
    with gated() as g:
        got = im.stats()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(got, want, equal_nan=equal_nan), (what, got, want)
    assert g.ran == {kernel: 1} if kernel else sum(g.ran.values()) == 1, (what, g.ran)
    # the single numbers are the matrix's row 0
    value, where = im.min(with_options=True)
    assert np.array_equal([value, where["x"], where["y"]], got[0, [0, 6, 7]], equal_nan=equal_nan), what
    value, where = im.max(with_options=True)
    assert np.array_equal([value, where["x"], where["y"]], got[0, [1, 8, 9]], equal_nan=equal_nan), what
    assert np.array_equal([im.avg(), im.deviate()], got[0, [4, 5]], equal_nan=equal_nan), what
    assert im.min() == got[0, 0] and im.max() == got[0, 1]
    return got


def spanning_width(dtype, bands):
    """A one-row image that spans three blocks of the kernel that takes it, the last one ragged."""
    threads, group = lib.vips_hip_arith_step(0), lib.vips_hip_arith_step(1)
    per_lane = group // np.dtype(dtype).itemsize if bands <= 4 else 1
    return 2 * threads * per_lane + 3 * per_lane + 1, threads * per_lane


@pytest.mark.parametrize("kernel", ["stream", "general"])
@pytest.mark.parametrize("bands", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("dtype", STATS_DTYPES, ids=lambda d: np.dtype(d).name)
def test_stats(dtype, bands, kernel):
    """All ten columns, sizes from one pel to several blocks, unique extremes at the first pel, the last pel and either
    side of a block's boundary.  Every sum is below 2^53, so the reference does not depend on its order either."""
    name = "stats_stream" if kernel == "stream" and bands <= 4 else "stats_general"
    with general_kernel(kernel == "general"):
        wide, boundary = spanning_width(dtype, bands if kernel == "stream" else 5)
        for w, h in ((1, 1), (7, 5), (300, 40), (wide, 1), (wide // 3 + 1, 3)):
            n = w * h
            spots = [(0, n - 1), (n - 1, 0)]
            if n > boundary + bands:
                spots += [(boundary - bands, boundary + bands - 1), (boundary, boundary - 1)]
            for pel_min, pel_max in spots:
                src = quiet(w, h, dtype, bands, 100 + w)
                if n >= 2 * bands:
                    place(src, pel_min, pel_max)
                check_stats(src, (np.dtype(dtype).name, bands, w, h, pel_min, pel_max), kernel=name, equal_nan=n == 1)


@pytest.mark.parametrize("kernel", ["stream", "general"])
@pytest.mark.parametrize("dtype", [np.uint16, np.int16], ids=lambda d: np.dtype(d).name)
def test_stats_16_bit_range(dtype, kernel):
    """Noise over the whole 16-bit range: squares up to 2^32, negative shorts, the extremes 0 / 65535 and -32768 /
    32767.  300 x 40 pels keep every sum far below 2^53."""
    info = np.iinfo(dtype)
    rng = np.random.default_rng(231)
    for bands in (1, 3, 5):
        src = rng.integers(info.min + 10, info.max - 10, (40, 300, bands)).astype(dtype)
        flat = src.reshape(-1, bands)
        for k in range(bands):
            flat[4000 + 7 * k, k] = info.min + k
            flat[9000 - 5 * k, k] = info.max - k
        with general_kernel(kernel == "general"):
            got = check_stats(src, (np.dtype(dtype).name, bands), kernel="stats_stream" if kernel == "stream" and bands <= 4 else "stats_general")
        assert got[0, 0] == info.min and got[0, 1] == info.max and got[1, 3] == float((src[:, :, 0].astype(np.int64) ** 2).sum())


def test_stats_grid_stride():
    """More groups than the capped grid has lanes: a lane's second step.  Unique extremes in the second step against
    the reference; then equal extremes in both steps, of which the first in raster order is reported."""
    lanes = lib.vips_hip_arith_step(3) * lib.vips_hip_arith_step(0)
    for dtype, bands in ((np.uint8, 1), (np.float32, 4)):
        per_lane = lib.vips_hip_arith_step(1) // np.dtype(dtype).itemsize
        step = lanes * per_lane  # pels the grid takes in one step
        w = 2048
        h = (step + 40 * per_lane + 5) // w + 1
        assert -(-w * h // per_lane) > lanes
        src = quiet(w, h, dtype, bands, 241)
        flat = src.reshape(-1, bands)
        lo, hi = (-128, 127) if dtype == np.float32 else (0, 255)
        for k in range(bands):
            flat[w * h - 1 - k, k] = lo + k
            flat[step + 7 + k, k] = hi - k
        check_stats(src, ("stride", np.dtype(dtype).name), kernel="stats_stream")
        # the same extremes again, earlier in raster order but met by later lanes of the first step
        for k in range(bands):
            flat[16 * 1000 + k, k] = lo + k
            flat[16 * 300 + 3 + k, k] = hi - k
        got = Image.new_from_array(src).stats()
        for k in range(bands):
            assert (got[k + 1, 0], got[k + 1, 6] + w * got[k + 1, 7]) == (lo + k, 16 * 1000 + k), (dtype, k, got[k + 1])
            assert (got[k + 1, 1], got[k + 1, 8] + w * got[k + 1, 9]) == (hi - k, 16 * 300 + 3 + k), (dtype, k, got[k + 1])


@pytest.mark.parametrize("kernel", ["stream", "general"])
def test_stats_ties(kernel):
    """Of equal extremes the first in raster order: a constant image, and one whose extremes repeat."""
    with general_kernel(kernel == "general"):
        for dtype in (np.uint8, np.float32):
            wide, _ = spanning_width(dtype, 3)
            src = np.full((2, wide, 3), 7, dtype)
            got = Image.new_from_array(src).stats()
            assert (got[:, 0] == 7).all() and (got[:, 1] == 7).all() and (got[:, 6:] == 0).all(), got
            src[0, 5::97, 1] = 9
            src[1, 3::89, 2] = 2
            got = Image.new_from_array(src).stats()
            assert got[2, 1] == 9 and (got[2, 8], got[2, 9]) == (5, 0) and src[0, 5, 1] == 9
            assert got[3, 0] == 2 and (got[3, 6], got[3, 7]) == (3, 1) and src[1, 3, 2] == 2
            assert (got[0, 0], got[0, 6], got[0, 7]) == (2, 3, 1) and (got[0, 1], got[0, 8], got[0, 9]) == (9, 5, 0)


@pytest.mark.parametrize("kernel", ["stream", "general"])
def test_stats_nan(kernel):
    """A few NaNs, none at the start of a row (the reference's extremes start at the first value a thread meets): the
    extremes skip them and are the reference's; the sums are NaN on both sides."""
    src = quiet(300, 40, np.float32, 3, 201)
    place(src, 777, 5000)
    for y, x, k in ((0, 7, 0), (3, 150, 0), (39, 299, 1), (20, 33, 1)):
        src[y, x, k] = np.nan
    with general_kernel(kernel == "general"):
        got = check_stats(src, "nan", equal_nan=True)
    assert np.isnan(got[1, 2]) and np.isnan(got[2, 3]) and not np.isnan(got[3, 2:6]).any() and np.isnan(got[0, 2:6]).all()
    assert not np.isnan(got[:, [0, 1, 6, 7, 8, 9]]).any()


@pytest.mark.parametrize("kernel", ["stream", "general"])
def test_stats_float_sums(kernel):
    """Non-integer noise: sum and sum of squares against math.fsum of the same values within (N - 1) * 2^-53 * sum|x|,
    the bound of any double summation order; the extremes exactly; the same image twice gives the same bits."""
    src = noise(1031, 67, np.float32, 3, 211)
    with general_kernel(kernel == "general"):
        im = Image.new_from_array(src)
        got, again = im.stats(), im.stats()
    assert np.array_equal(got.view(np.uint64), again.view(np.uint64))
    u = 2.0 ** -53
    n = src.shape[0] * src.shape[1]
    for k in range(3):
        v = src[:, :, k].astype(np.float64).ravel()
        sq = v * v  # (a float's square is exact in double)
        assert abs(got[k + 1, 2] - math.fsum(v)) <= (n - 1) * u * math.fsum(np.abs(v)), k
        assert abs(got[k + 1, 3] - math.fsum(sq)) <= (n - 1) * u * math.fsum(sq), k
        assert got[k + 1, 0] == v.min() and got[k + 1, 1] == v.max()
        flat = src[:, :, k]
        assert flat[int(got[k + 1, 7]), int(got[k + 1, 6])] == v.min() and flat[int(got[k + 1, 9]), int(got[k + 1, 8])] == v.max()
    v = src.astype(np.float64).ravel()
    assert abs(got[0, 2] - math.fsum(v)) <= (v.size - 1) * u * math.fsum(np.abs(v))
    assert abs(got[0, 3] - math.fsum(v * v)) <= (v.size - 1) * u * math.fsum(v * v)


def test_stats_refusals():
    for dtype in (np.uint32, np.int32, np.float64):
        with pytest.raises(VipsHipError, match="outside the HIP path"):
            Image.new_from_array(noise(5, 4, dtype, 1, 221)).stats()


# ---------------------------------------------------------------- the libvips module

# (on host fibers the library under test is not the one the module was linked against)
needs_module = pytest.mark.skipif(not helpers.have_module() or bool(os.environ.get("VIPS_HIP_LIBRARY")),
                                  reason="host/_build missing, or another build of the library is under test")


@needs_module
@pytest.mark.parametrize("strips", [False, True], ids=["whole", "strips"])
def test_module_arith_classes(strips):
    """linear_hip, invert_hip and abs_hip make the built-in operations' pixels, whole and strip by strip (a small
    $VIPS_HIP_BUDGET, as tests/test_module.py)."""
    Ref.load_module()
    module = ctypes.CDLL(helpers.MODULE_LIB)
    height = 700 if strips else 50
    rgba = noise(400, height, np.uint8, 4, 301)
    grey = noise(400, height, np.uint16, 1, 303)
    signed = noise(400, height, np.int16, 3, 305, with_extremes=True)
    cases = [("linear", rgba, "a=1.1,b=-20.3"), ("linear", rgba, "a=1.1 1.1 -2.5 0.3,b=-20.3 7.25 300 7.25"),
             ("linear", rgba, "a=1.1 1.1 -2.5 0.3,b=-20.3,uchar=true"), ("linear", rgba, "a=-1.5,b=300,uchar=true"),
             ("linear", grey, "a=0.004 0.004 -0.01,b=-5.3 7.25 300"), ("linear", signed, "a=0.01,b=0.5"),
             ("invert", rgba, ""), ("invert", signed, ""), ("abs", signed, ""), ("abs", grey, "")]
    if strips:
        os.environ["VIPS_HIP_BUDGET"] = "300k"
    before = module.vips_hip_module_strips_done()
    try:
        for nick, src, args in cases:
            same(Ref.run(nick + "_hip", src, args, interpretation=INTERP["srgb"]),
                 Ref.run(nick, src, args, interpretation=INTERP["srgb"]), "%s_hip %s" % (nick, args))
    finally:
        if strips:
            del os.environ["VIPS_HIP_BUDGET"]
    if strips:
        assert module.vips_hip_module_strips_done() - before >= 4 * len(cases), "not strip-mined"


@needs_module
def test_module_errors_are_the_originals():
    Ref.load_module()
    src = noise(40, 30, np.uint8, 3, 307)
    with pytest.raises(RuntimeError, match="vector must have 1 or 3 elements"):
        Ref.run("linear_hip", src, "a=1 2,b=0")
