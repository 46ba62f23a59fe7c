"""GPU parity: vips_round, vips_sign, vips_clamp, vips_minpair, vips_maxpair, vips_remainder and vips_remainder_const on
the device (the policies of libvips_amd/csrc/arith.hip behind ops_arith.cpp's new entry points).

Every comparison is equality of dtype, shape, interpretation and bits against the compiled reference -- float and
double results as their integer views, so that -0.0 is not +0.0 -- with one exception: positions where both sides are
NaN count as equal (the host's and the device's default NaN differ in sign).  Nothing has a tolerance.  One-image
operations reach the reference through Ref.run, two-image operations through its command line.  Every case asserts by
the gate report which kernel ran and that it was launched once, on the streaming kernel and on the one-element-a-lane
kernel that VIPS_HIP_NO_ARITH_STREAM forces.

Kept out of the inputs, because the reference's own behaviour there is undefined (include/vips_hip.h says what the
device does instead): INT_MIN % -1, clamp bounds outside an integer format's range, and minpair / maxpair of zeros of
opposite sign -- the compiled reference answers +0.0 or -0.0 by the order of its operands there
(test_pair_of_opposite_zeros_is_not_pinned shows it), so there is nothing to pin.
Runs on the CPU too, on host fibers (tests/test_emul_arith2.py)."""
import ctypes

import numpy as np
import pytest

import libvips_amd
from libvips_amd import Image, VipsHipError, _ffi
from tests import helpers
from tests.helpers import Ref
from tests.test_arith_gpu import ALL_DTYPES, extremes_of, gated, gen_in_frames, general_kernel, noise, ref_cli

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not helpers.have_ref(), reason="oracle/_ref not built")]

lib = _ffi.lib
INTERP = helpers.INTERP
KERNELS = ["stream", "general"]
FLOATS = [np.float32, np.float64]
W, H, BANDS = 21, 9, 3  # 567 elements: no multiple of any group of the streaming kernel


def name_of(dtype):
    return np.dtype(dtype).name


@pytest.fixture(scope="module", autouse=True)
def _init():
    libvips_amd.init(0)


def same_bits(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    if got.dtype.kind == "f":
        view = np.uint32 if got.dtype.itemsize == 4 else np.uint64
        both_nan = np.isnan(got) & np.isnan(want)
        got, want = np.where(both_nan, 0, got.view(view)), np.where(both_nan, 0, want.view(view))
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (what, bad[:4].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


def check_one(nick, src, args, fn, kernel, what, interp=INTERP["srgb"], launches=1):
    """A one-image operation against Ref.run: bits, header, and which kernel ran."""
    want, want_interp = Ref.run_interp(nick, src, args, interpretation=interp)
    with general_kernel(kernel == "general"), gated() as g:
        out = fn(Image.new_from_array(src, interp))
        got = out.numpy()
    same_bits(got, want, (nick, args, what, kernel))
    assert lib.vips_hip_image_get_interpretation(out._h) == want_interp, (nick, what)
    assert g.ran == ({"arith_" + kernel: 1} if launches else {}), (nick, what, g.ran)


def check_two(tmp_path, op, a, b, kernel, what, ran=None):
    """A two-image operation against the reference's command line.  a, b: (array, interpretation)."""
    want, want_interp = ref_cli(tmp_path, op, [a, b])
    with general_kernel(kernel == "general"), gated() as g:
        out = getattr(Image.new_from_array(*a), op)(Image.new_from_array(*b))
        got = out.numpy()
    same_bits(got, want, (op, what, kernel))
    assert lib.vips_hip_image_get_interpretation(out._h) == want_interp, (op, what)
    # ONE launch, whatever had to be matched
    assert g.ran == {"arith_" + (ran or kernel): 1}, (op, what, g.ran)


def with_specials(dtype, specials, seed):
    """Noise with the format's extremes, then `specials`, at its start."""
    src = noise(W, H, dtype, BANDS, seed, with_extremes=True)
    flat = src.ravel()
    n = len(extremes_of(dtype))
    flat[n:n + len(specials)] = np.asarray(specials, dtype)
    return src


# ---------------------------------------------------------------- round

ROUND_VALUES = [0.5, -0.5, 1.5, -1.5, 2.5, -2.5, -0.3, 0.0, -0.0, 2.0 ** 23 + 1, np.inf, -np.inf, np.nan]


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("kind", ["rint", "ceil", "floor"])
@pytest.mark.parametrize("dtype", FLOATS, ids=name_of)
def test_round(dtype, kind, kernel):
    src = with_specials(dtype, ROUND_VALUES, 501)
    check_one("round", src, "round=" + kind, lambda im: im.round(kind), kernel, name_of(dtype))


def test_round_of_an_integer_image_is_a_copy():
    """round.c:77-79: no kernel runs."""
    for dtype in (np.uint8, np.int32):
        src = noise(W, H, dtype, BANDS, 503, with_extremes=True)
        check_one("round", src, "round=ceil", lambda im: im.ceil(), "stream", name_of(dtype), launches=0)
    src = with_specials(np.float32, ROUND_VALUES, 505)
    im = Image.new_from_array(src)
    for kind in ("rint", "ceil", "floor"):
        same_bits(getattr(im, kind)().numpy(), Ref.run("round", src, "round=" + kind), kind)


# ---------------------------------------------------------------- sign

@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("dtype", ALL_DTYPES, ids=name_of)
def test_sign(dtype, kernel):
    """The format's extremes; both zeros and NaN (which is -1: neither > 0 nor == 0) for the float formats."""
    specials = [0.0, -0.0, np.nan, -np.nan] if np.dtype(dtype).kind == "f" else [0, 1]
    src = with_specials(dtype, specials, 511)
    check_one("sign", src, "", lambda im: im.sign(), kernel, name_of(dtype))
    if np.dtype(dtype).kind == "f":
        n = len(extremes_of(dtype))
        got = Image.new_from_array(src).sign().numpy().ravel()[n:n + 4]
        assert got.dtype == np.int8 and got.tolist() == [0, 0, -1, -1]


# ---------------------------------------------------------------- clamp

def clamp_cases(dtype):
    """(min, max) or None for the defaults; every bound inside the format's range."""
    cases = [None, (10.0, 100.0), (100.0, 10.0)]  # the defaults, inside the range, min > max
    if dtype == np.uint8:
        cases += [(1.5, 200.7)]  # fractional bounds are truncated at the store
    if np.dtype(dtype).kind == "i":
        cases += [(-20.5, 33.9)]
    if np.dtype(dtype).kind == "f":
        cases += [(0.1, 0.7), (-0.3, 1e-3)]  # bounds that are no floats
    return cases


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("dtype", ALL_DTYPES, ids=name_of)
def test_clamp(dtype, kernel):
    """NaN pels come through (the float formats)."""
    specials = [np.nan, 0.5, 0.1, 0.7, 0.70000005, -0.0] if np.dtype(dtype).kind == "f" else [0, 1, 2, 10, 100, 101]
    src = with_specials(dtype, specials, 521)
    for case in clamp_cases(dtype):
        if case is None:
            check_one("clamp", src, "", lambda im: im.clamp(), kernel, (name_of(dtype), "defaults"))
        else:
            lo, hi = case
            check_one("clamp", src, "min=%r,max=%r" % (lo, hi), lambda im: im.clamp(min=lo, max=hi), kernel, (name_of(dtype), case))


# ---------------------------------------------------------------- minpair, maxpair

def pair_operands(dtype, seed, shape_a=(W, H, BANDS), shape_b=(W, H, BANDS), extremes=True):
    a = noise(*shape_a[:2], dtype, shape_a[2], seed, with_extremes=extremes)
    b = noise(*shape_b[:2], dtype, shape_b[2], seed + 2)
    if extremes:
        # ties, in both the formats' kinds
        b.ravel()[20:24] = a.ravel()[20:24]
    return a, b


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("op", ["minpair", "maxpair"])
@pytest.mark.parametrize("dtype", ALL_DTYPES, ids=name_of)
def test_pair(tmp_path, dtype, op, kernel):
    a, b = pair_operands(dtype, 531)
    if np.dtype(dtype).kind == "f":
        # NaN against a number in both orders, NaN against NaN; the zeros of `a` meet numbers that are not zero
        a.ravel()[30:33] = [np.nan, 3.5, np.nan]
        b.ravel()[30:33] = [2.5, np.nan, np.nan]
        n = len(extremes_of(dtype))
        assert (b.ravel()[:n] != 0).all()
    check_two(tmp_path, op, (a, INTERP["srgb"]), (b, INTERP["srgb"]), kernel, name_of(dtype))
    check_two(tmp_path, op, (b, INTERP["srgb"]), (a, INTERP["srgb"]), kernel, (name_of(dtype), "swapped"))


@pytest.mark.parametrize("op", ["minpair", "maxpair", "remainder"])
def test_two_images_are_matched(tmp_path, op):
    """vips__formatalike, vips__bandalike (one band against three, indexed by pel) and vips__sizealike (zero outside an
    image's own rectangle): one launch of the one-element-a-lane kernel, no bandjoin or embed."""
    for dtype in (np.uint8, np.int16, np.float32):
        one, three = pair_operands(dtype, 541, (W, H, 1), (W, H, 3), extremes=False)
        check_two(tmp_path, op, (one, INTERP["b-w"]), (three, INTERP["srgb"]), "stream", (name_of(dtype), "1 against 3"), ran="general")
        check_two(tmp_path, op, (three, INTERP["srgb"]), (one, INTERP["b-w"]), "stream", (name_of(dtype), "3 against 1"), ran="general")
        a, b = pair_operands(dtype, 543, (7, 5, 3), (4, 9, 3), extremes=False)
        # (no negative zero against the zeros an image reads outside itself)
        check_two(tmp_path, op, (a, INTERP["srgb"]), (b, INTERP["srgb"]), "stream", (name_of(dtype), "sizes"), ran="general")
        check_two(tmp_path, op, (b, INTERP["srgb"]), (a, INTERP["srgb"]), "stream", (name_of(dtype), "sizes, swapped"), ran="general")
    # the common format: uchar and short meet in short, short and float in float
    a, _ = pair_operands(np.uint8, 545)
    b, _ = pair_operands(np.int16, 547, extremes=False)
    c, _ = pair_operands(np.float32, 549, extremes=False)
    b[b == 0] = 3
    c[c == 0] = 3
    check_two(tmp_path, op, (a, INTERP["srgb"]), (b, INTERP["srgb"]), "stream", "uchar, short")
    check_two(tmp_path, op, (c, INTERP["srgb"]), (b, INTERP["srgb"]), "stream", "float, short")


def test_pair_of_opposite_zeros_is_not_pinned(tmp_path):
    """The compiled reference's fmin / fmax of +0.0 and -0.0 follow the order of the operands, so that corner has no
    reference; the device's answer is the same in both orders: -0.0 is the smaller."""
    pz, nz = np.zeros((1, 4, 1), np.float32), np.full((1, 4, 1), -0.0, np.float32)
    ref = [ref_cli(tmp_path, "minpair", [(x, INTERP["b-w"]), (y, INTERP["b-w"])])[0] for x, y in ((pz, nz), (nz, pz))]
    assert not np.array_equal(np.signbit(ref[0]), np.signbit(ref[1]))
    for dtype in FLOATS:
        p, n = Image.new_from_array(pz.astype(dtype)), Image.new_from_array(nz.astype(dtype))
        for x, y in ((p, n), (n, p)):
            assert np.signbit(x.minpair(y).numpy()).all() and not np.signbit(x.maxpair(y).numpy()).any()


# ---------------------------------------------------------------- remainder, remainder_const

def remainder_operands(dtype, seed):
    """Negative operands, zero divisors, the extremes on the left; never INT_MIN against -1."""
    a = noise(W, H, dtype, BANDS, seed, with_extremes=True)
    b = noise(W, H, dtype, BANDS, seed + 2)
    if np.dtype(dtype).kind == "f":
        b.ravel()[5::7] = 0.0
        b.ravel()[6::14] = -0.0
        # inexact quotients
        a.ravel()[40:44] = [7.3, -7.3, 1e10, 0.3]
        b.ravel()[40:44] = [0.1, 0.1, 0.7, -0.1]
    else:
        if np.dtype(dtype).kind == "i":
            b[b == -1] = -7
        small = noise(W, H, dtype, BANDS, seed + 4) % 11  # divisors that leave something
        b.ravel()[1::2] = small.ravel()[1::2]
        if np.dtype(dtype).kind == "i":
            b.ravel()[3::8] = -5
        b.ravel()[5::7] = 0
    return a, b


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("dtype", ALL_DTYPES, ids=name_of)
def test_remainder(tmp_path, dtype, kernel):
    a, b = remainder_operands(dtype, 551)
    check_two(tmp_path, "remainder", (a, INTERP["srgb"]), (b, INTERP["srgb"]), kernel, name_of(dtype))


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("dtype", ALL_DTYPES, ids=name_of)
def test_remainder_const(dtype, kernel):
    """One constant and one a band, a zero constant (-1: the format's maximum where it is unsigned), a negative one, a
    fractional one (it becomes c_int: 2.7 is 2)."""
    src = with_specials(dtype, [7.3, -7.3, 0.3, 2.7] if np.dtype(dtype).kind == "f" else [0, 1, 2, 7], 561)
    for c in ([7], [2.7], [0], [-3], [3, 0, 5], [2.7, -4.2, 1]):
        args = "c=" + " ".join(repr(float(v)) for v in c)
        check_one("remainder_const", src, args, lambda im: im.remainder(c if len(c) > 1 else c[0]), kernel, (name_of(dtype), c))


def test_remainder_const_bands_up_and_operator():
    """A one-band image against three constants makes three bands: the one-element-a-lane kernel, the input indexed by
    pel; `%` is remainder."""
    src = noise(W, H, np.uint8, 1, 563, with_extremes=True)
    check_one("remainder_const", src, "c=3 0 5", lambda im: im % [3, 0, 5], "general", "1 band against 3", interp=INTERP["b-w"])
    a, b = remainder_operands(np.int16, 565)
    same_bits((Image.new_from_array(a) % Image.new_from_array(b)).numpy(), Image.new_from_array(a).remainder(Image.new_from_array(b)).numpy(), "%")
    with pytest.raises(RuntimeError) as ref:
        Ref.run("remainder_const", noise(W, H, np.uint8, 3, 567), "c=1 2")
    with pytest.raises(VipsHipError) as dev:
        Image.new_from_array(noise(W, H, np.uint8, 3, 567)).remainder([1, 2])
    assert str(ref.value).strip().split(": ")[-1] in str(dev.value)


# ---------------------------------------------------------------- refusals, the region forms

def test_complex_images_are_refused():
    z = (noise(5, 4, np.float32, 1, 571) + 1j * noise(5, 4, np.float32, 1, 573)).astype(np.complex64)
    for fn in (lambda i: i.round("rint"), lambda i: i.sign(), lambda i: i.clamp(), lambda i: i.minpair(i), lambda i: i.maxpair(i),
               lambda i: i.remainder(i), lambda i: i.remainder(3)):
        with pytest.raises(VipsHipError, match="image must be non-complex"):
            fn(Image.new_from_array(z))
    with pytest.raises(VipsHipError, match="round: bad operation 3"):
        Image.new_from_array(noise(5, 4, np.float32, 1, 575)).round(3)


@pytest.mark.parametrize("kernel", ["stream", "general", "unaligned"])
def test_region_forms(kernel):
    """The generate functions on windows of larger frames, whole and strip by strip with strips of one row: the bytes of
    the whole-image call, nothing written outside the window.  unaligned: rows one element off a dword, which the
    streaming kernel declines for elements smaller than one."""
    c = (ctypes.c_double * 3)(3, 0, 5)
    forms = [("round", np.float32, np.float32, lambda i, o: lib.vips_hip_round_gen(2, i, o), lambda im: im.floor()),
             ("sign", np.int16, np.int8, lib.vips_hip_sign_gen, lambda im: im.sign()),
             ("clamp", np.uint8, np.uint8, lambda i, o: lib.vips_hip_clamp_gen(1.5, 200.7, i, o), lambda im: im.clamp(1.5, 200.7)),
             ("remainder_const", np.uint16, np.uint16, lambda i, o: lib.vips_hip_remainder_const_gen(c, 3, i, o),
              lambda im: im.remainder([3, 0, 5]))]
    margin = 1 if kernel == "unaligned" else 4
    for name, dtype, out_dtype, gen, whole in forms:
        src = noise(W, H, dtype, BANDS, 581, with_extremes=True)
        want = whole(Image.new_from_array(src)).numpy()
        streams = kernel == "stream" or (kernel == "unaligned" and min(np.dtype(dtype).itemsize, np.dtype(out_dtype).itemsize) >= 4)
        with general_kernel(kernel == "general"), gated() as g:
            got = gen_in_frames(src, out_dtype, BANDS, gen, margin)
        assert g.ran == {"arith_stream" if streams else "arith_general": 1}, (name, g.ran)
        same_bits(got, want, (name, kernel))
        rows = [gen_in_frames(src[y:y + 1], out_dtype, BANDS, gen, margin) for y in range(H)]
        same_bits(np.concatenate(rows, axis=0), want, (name, kernel, "strips of one row"))
