"""The library's DEFAULT float mode (vips_hip_set_exact_float(0): what bench.py, the libvips module and every user get),
which the rest of the suite pins away (tests/conftest.py runs every test in the exact mode).

In the default mode the large float convolutions of integer images (conv.hip: convf_rows_lds<.., FUSED> and
convf_grouped<.., FUSED>, masks 8 or more wide) and the streaming separable convolution of float images
(convsep_stream.hip MODE 3) sum with fused multiply-adds.  include/vips_hip.h promises: at most 1 ULP from the
reference where the taps are of one sign and the pels under a window are of one sign; masks whose taps differ in sign
always get the exact arithmetic; operations a decision hangs on (canny, smartcrop's attention search) ask for the exact
arithmetic themselves.

Two host chains stand beside the device (section A): chain_mul_add, the reference's float64 `s = s + c * p` in
row-major mask order over the edge-clamped window (convf.c:163-181), and chain_fma, the same with ONE rounding per tap,
computed exactly.  conv.hip documents that its fused kernels keep that order (zero padding taps multiplied through:
exact), so in the default mode the device must give chain_fma's bits, not only something within 1 ULP -- a lane that
took a wrong tap or pel shows there.  chain_fma is slow (exact integer arithmetic in Python), so it runs on a sample of
the outputs: the first and last pel of every row, both sides of every block seam (every 2048 columns of the LDS
kernel, every 256 x CONV_TILE = 2048 elements of the grouped one), some of the first and last row, a seeded random
couple of hundred, and the outputs whose double sum lies nearest a float rounding boundary -- the ones where one
rounding per tap instead of two can show at all.  On noise the two chains' doubles differ at a third of the outputs but
store the same FLOAT on every sampled output of the Gaussian masks below, so every sweep also holds a mask whose offset
aims one output's sum at a rounding boundary (aimed_offset): there the chains part, and the test says so.

No tolerance but the project's own appears: bit equality, or the 1 ULP of BASELINE.json's north_star.  The shapes are
the smallest at which the kernels take another path: see each test."""
import contextlib
import ctypes
import math
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import libvips_amd
from libvips_amd import Image, _ffi
from tests import helpers
from tests.helpers import PortCC, Ref
from tests.test_conv_colour_gpu import ulp_distance
from tests.test_edge_gpu import canny_tile, check_canny, gated, noise, ranged, same

lib = _ffi.lib
gpu = pytest.mark.gpu
needs_ref = pytest.mark.skipif(not helpers.have_ref(), reason="oracle/_ref not built")

SEAM = 2048  # conv.hip: CONVF_LDS_SPAN columns a block of the LDS kernel; 256 lanes x CONV_TILE elements of the grouped one
UNSIGNED = {np.dtype(np.int8): np.uint8, np.dtype(np.int16): np.uint16, np.dtype(np.int32): np.uint32}


@pytest.fixture(scope="module")
def device():
    libvips_amd.init(0)


@contextlib.contextmanager
def default_mode():
    """The shipped float mode inside, the suite's exact mode behind it again."""
    assert lib.vips_hip_get_exact_float() == 1
    lib.vips_hip_set_exact_float(0)
    try:
        yield
    finally:
        lib.vips_hip_set_exact_float(1)


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def same_bits(got, want, what):
    assert got.dtype == np.float32 and want.dtype == np.float32 and got.shape == want.shape, (what, got.dtype, got.shape)
    bad = np.argwhere(bits(got) != bits(want))
    assert len(bad) == 0, "%s: %d of %d differ, first at %s: got %r want %r" % (
        what, len(bad), got.size, bad[0], got[tuple(bad[0])], want[tuple(bad[0])])


def image(w, h, bands, dtype, seed, both_signs=False):
    """LCG noise of the whole range of the format; the signed formats keep to non-negative pels unless asked."""
    a = helpers.lcg_image(w, h, bands, dtype, seed)
    if np.dtype(dtype).kind == "i" and not both_signs:
        a = (a.view(UNSIGNED[np.dtype(dtype)]) >> 1).astype(dtype)
    return np.ascontiguousarray(a)


_gauss = {}


def gauss_mask(mw, mh):
    """(mask, scale): the centre mh x mw of a float Gaussian of libvips_amd.gaussmat wide enough to hold it, and its sum."""
    if (mw, mh) not in _gauss:
        sigma = max(mw, mh) / 6.0 + 0.4
        while True:
            m, _ = libvips_amd.gaussmat(sigma, 0.01, False, "float")
            if m.shape[0] >= max(mw, mh):
                break
            sigma *= 1.25
        y0, x0 = (m.shape[0] - mh) // 2, (m.shape[1] - mw) // 2
        crop = np.ascontiguousarray(m[y0:y0 + mh, x0:x0 + mw])
        assert (crop > 0).all() and crop.shape == (mh, mw)
        _gauss[(mw, mh)] = (crop, float(crop.sum()))
    return _gauss[(mw, mh)]


def random_mask(mw, mh, seed):
    """A positive fractional mask with a scale of its own."""
    rng = np.random.RandomState(seed)
    return np.ascontiguousarray(rng.uniform(0.05, 1.0, size=(mh, mw))), 3.7


# ---------------------------------------------------------------- A. the two host chains

def coefficients(mask, scale):
    """convf.c:300-323: the scale is baked into the mask."""
    m = np.asarray(mask, dtype=np.float64)
    if m.ndim == 1:
        m = m[None, :]
    return m / scale


def padded(src, mh, mw):
    """vips_embed(VIPS_EXTEND_COPY) of convf.c:331-336: out(x, y) reads in(x + i - mw / 2, y + j - mh / 2), clamped."""
    return np.pad(src, ((mh // 2, mh - 1 - mh // 2), (mw // 2, mw - 1 - mw // 2), (0, 0)), mode="edge")


def chain_mul_add(src, mask, scale, offset, store=True):
    """The reference's arithmetic on the whole image: float64 `s = s + c * p`, two roundings a tap (numpy does not
    contract), the non-zero taps in row-major mask order, seeded with the offset; stored as float (store=False: the
    doubles)."""
    coef = coefficients(mask, scale)
    mh, mw = coef.shape
    h, w, _ = src.shape
    pad = padded(src, mh, mw).astype(np.float64)  # (exact: pels of at most 32 bits)
    s = np.full(src.shape, float(offset), np.float64)
    for j in range(mh):
        for i in range(mw):
            if coef[j, i] != 0.0:
                s = s + coef[j, i] * pad[j:j + h, i:i + w]
    return s.astype(np.float32) if store else s


_TWO53 = 9007199254740992.0


def fma_exact(c, p, s):
    """round(c * p + s) with ONE rounding, for doubles c and s and an integer p (math.fma where the interpreter has it).
    c and s are m * 2^e with integer m, so c * p + s is an integer times a power of two; Python's int -> float
    conversion rounds to nearest even, and ldexp of a normal result is exact."""
    if hasattr(math, "fma"):
        return math.fma(c, float(p), s)
    m, e = math.frexp(c)
    mc, ec = int(m * _TWO53), e - 53
    m, e = math.frexp(s)
    ms, es = int(m * _TWO53), e - 53
    if es >= ec:
        return math.ldexp(float((ms << (es - ec)) + mc * p), ec)
    return math.ldexp(float(ms + ((mc * p) << (ec - es))), es)


def gather(src, mask, scale, ys, es):
    """(the non-zero coefficients in row-major mask order, for every output (ys[k], element es[k] of the row) the pels
    under them as Python ints)."""
    coef = coefficients(mask, scale)
    mh, mw = coef.shape
    bands = src.shape[2]
    pad = padded(src, mh, mw)
    jj, ii = np.nonzero(coef)  # (row-major)
    xs, bs = np.divmod(np.asarray(es), bands)
    ys = np.asarray(ys)
    pels = pad[ys[:, None] + jj[None, :], xs[:, None] + ii[None, :], bs[:, None]].astype(np.int64).tolist()
    return coef[jj, ii].tolist(), pels


def chain_mul_add_at(src, mask, scale, offset, ys, es, store=True):
    """chain_mul_add at single outputs (Python's float is the IEEE double, `s + c * p` two operations)."""
    cs, pels = gather(src, mask, scale, ys, es)
    out = np.empty(len(pels), np.float64)
    for k, row in enumerate(pels):
        s = float(offset)
        for c, p in zip(cs, row):
            s = s + c * p
        out[k] = s
    return out.astype(np.float32) if store else out


def chain_fma(src, mask, scale, offset, ys, es, store=True):
    """The same sum with one rounding per tap (the device's __fma_rn) at the outputs (ys[k], element es[k] of the
    row), stored as float (store=False: the doubles)."""
    cs, pels = gather(src, mask, scale, ys, es)
    out = np.empty(len(pels), np.float64)
    if hasattr(math, "fma"):
        for k, row in enumerate(pels):
            s = float(offset)
            for c, p in zip(cs, row):
                s = math.fma(c, float(p), s)
            out[k] = s
        return out.astype(np.float32) if store else out
    split = []
    for c in cs:
        m, e = math.frexp(c)
        split.append((int(m * _TWO53), e - 53))
    frexp, ldexp = math.frexp, math.ldexp
    for k, row in enumerate(pels):
        s = float(offset)
        for (mc, ec), p in zip(split, row):  # (fma_exact, inlined: this loop is the cost of the file)
            if p:
                m, e = frexp(s)
                e -= 53
                if e >= ec:
                    s = ldexp(float((int(m * _TWO53) << (e - ec)) + mc * p), ec)
                else:
                    s = ldexp(float(int(m * _TWO53) + ((mc * p) << (ec - e))), e)
        out[k] = s
    return out.astype(np.float32) if store else out


def near_boundaries(sums, k=8):
    """The k outputs whose double sum lies nearest a rounding boundary of float: where the last bits of the double
    decide the float."""
    f = sums.astype(np.float32)
    ulp = np.spacing(np.abs(f)).astype(np.float64)
    away = 0.5 - np.abs(sums - f.astype(np.float64)) / ulp
    flat = np.argsort(away.reshape(-1), kind="stable")[:k]
    ne = sums.shape[1] * sums.shape[2]
    return [(int(i // ne), int(i % ne)) for i in flat]


def sample_points(shape, seed, extra=(), n_random=150, seam_origin=0):
    """(ys, es): the sample of outputs chain_fma runs on -- see the head of the file.  seam_origin: the element of the
    row the kernel's first block starts at (region form: 0 of the OUTPUT rect, which is what `shape` is)."""
    h, w, bands = shape
    ne = w * bands
    rng = np.random.RandomState(seed)
    cols = set(range(bands)) | set(range(ne - bands, ne))
    for s in range(seam_origin + SEAM, ne, SEAM):
        cols |= {s - 1, s}
    pts = {(y, e) for y in range(h) for e in cols}
    for y in (0, h - 1):
        pts |= {(y, int(e)) for e in rng.randint(0, ne, 16)}
    pts |= {(int(y), int(e)) for y, e in zip(rng.randint(0, h, n_random), rng.randint(0, ne, n_random))}
    pts |= set(extra)
    pts = sorted(pts)
    return np.array([p[0] for p in pts]), np.array([p[1] for p in pts])


def aimed_offset(src, mask, scale, offset, y, e, count=96):
    """(offset', (y, e')): an offset near `offset` that puts the reference's double sum of one output on the boundary
    between two floats -- the one place where one rounding per tap and two can store different floats -- and that
    output: the first of row y, from element e on, at which the two host chains then do store different floats.
    (The offset seeds the sum, convf.c:165, so it moves every output by the same amount; the chains' doubles differ
    at about a third of the outputs, by an ulp or two, and a sum ON the boundary goes to the even float, so about one
    candidate in six parts them.  The search is the host's own arithmetic: the device has no part in it.)"""
    es = np.arange(e, min(e + count, src.shape[1] * src.shape[2]))
    ys = np.full(len(es), y)
    two = chain_mul_add_at(src, mask, scale, offset, ys, es, store=False)
    one = chain_fma(src, mask, scale, offset, ys, es, store=False)
    for k in np.nonzero(two != one)[0]:
        f = np.float32(two[k])
        other = np.nextafter(f, np.float32(np.inf) if float(f) <= two[k] else np.float32(-np.inf))
        aimed = offset + ((float(f) + float(other)) / 2.0 - two[k])
        at = (ys[k:k + 1], es[k:k + 1])
        if bits(chain_fma(src, mask, scale, aimed, *at))[0] != bits(chain_mul_add_at(src, mask, scale, aimed, *at))[0]:
            return float(aimed), (y, int(es[k]))
    raise AssertionError("no output of row %d parts the chains" % y)


def reference(src, mask, scale, offset):
    return PortCC.conv(src, mask, scale, offset, "float")


def run_conv(src, mask, scale, offset):
    return Image.new_from_array(src).conv(mask, scale=scale, offset=offset, precision="float").numpy()


def check_conv(src, mask, scale=1.0, offset=0.0, seed=1, what="", fused=True, contract=True):
    """One input through the device in both modes against the reference and the two host chains.
    exact mode == reference, bit for bit; the default mode:
      fused=False (the fused kernels do not take this input): == reference, bit for bit;
      fused=True: (a) within 1 ULP of the reference on the whole output (contract=False: pels of both signs, outside
                  the header's bound), (b) == chain_fma bit for bit on the sample.
    Returns how many sampled outputs chain_fma and chain_mul_add store differently."""
    what = "%s %s %s mask %s" % (what, src.shape, src.dtype, np.asarray(mask).shape)
    want = reference(src, mask, scale, offset)
    sums = chain_mul_add(src, mask, scale, offset, store=False)
    same_bits(sums.astype(np.float32), want, "chain_mul_add against the port, " + what)
    exact = run_conv(src, mask, scale, offset)
    same_bits(exact, want, "exact mode, " + what)
    with default_mode():
        fast = run_conv(src, mask, scale, offset)
    if not fused:
        same_bits(fast, want, "default mode, nothing fused, " + what)
        return 0
    assert fast.dtype == np.float32 and fast.shape == want.shape
    if contract:
        assert ulp_distance(fast, want) <= 1, what  # tolerance: 1 ULP (BASELINE.json north_star)
    h = src.shape[0]
    ys, es = sample_points(src.shape, seed, extra=near_boundaries(sums))
    fm = chain_fma(src, mask, scale, offset, ys, es)
    got = fast.reshape(h, -1)[ys, es]
    bad = np.nonzero(bits(got) != bits(fm))[0]
    assert len(bad) == 0, "default mode against chain_fma, %s: %d of %d sampled differ, first at (y %d, e %d): got %r want %r" % (
        what, len(bad), len(ys), ys[bad[0]], es[bad[0]], got[bad[0]], fm[bad[0]])
    return int((bits(fm) != bits(want.reshape(h, -1)[ys, es])).sum())


def check_aimed(src, mw, mh, seed, start, what, **kwargs):
    """The random positive mask with a scale and an offset aimed at an output (aimed_offset, searched from `start`
    on) through check_conv: the count of sampled outputs at which the chains part -- the aimed one is in the sample, as
    the output nearest a boundary -- which is 1 or more."""
    mask, scale = random_mask(mw, mh, seed)
    offset, target = aimed_offset(src, mask, scale, 11.25, *start)
    assert offset != 0.0
    n = check_conv(src, mask, scale, offset, seed, what + " aimed at %r" % (target,), **kwargs)
    assert n >= 1, (what, target, n)
    return n


def test_fma_exact_against_rationals():
    """fma_exact against exact rationals (float() of a Fraction rounds correctly): random operands, sums that cancel,
    ties."""
    rng = np.random.RandomState(5)
    cases = []
    for _ in range(3000):
        c = float(rng.uniform(-1, 1) * 2.0 ** rng.randint(-40, 10))
        p = int(rng.randint(-2 ** 31, 2 ** 31))
        s = float(rng.uniform(-1, 1) * 2.0 ** rng.randint(-40, 50))
        cases.append((c, p, s))
        cases.append((c, p, -c * p))  # cancels down to the rounding error of the product
        cases.append((c, p, -c * p * (1 + 2.0 ** -30)))
    cases += [(2.0 ** -53, 1, 1.0), (2.0 ** -53, 3, 1.0), (2.0 ** -54, 3, 1.0), (0.1, 0, 7.5), (0.1, 10, 0.0), (0.0, 9, 0.0)]
    for c, p, s in cases:
        want = float(Fraction(c) * p + Fraction(s))
        got = fma_exact(c, p, s)
        assert got == want, (c, p, s, got, want)
    # and chain_fma's own loop, on pels of both signs under a mask of both signs (sums that cancel)
    src = image(23, 7, 2, np.int32, 6, both_signs=True)
    mask, scale = random_mask(9, 3, 7)
    mask -= 0.5
    ys, es = sample_points(src.shape, 8, n_random=20)
    cs, pels = gather(src, mask, scale, ys, es)
    got = chain_fma(src, mask, scale, -1.75, ys, es, store=False)
    for k, row in enumerate(pels):
        s = -1.75
        for c, p in zip(cs, row):
            s = float(Fraction(c) * p + Fraction(s))
        assert got[k] == s, (k, got[k], s)


@pytest.mark.parametrize("dtype", [np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32], ids=lambda d: np.dtype(d).name)
def test_chain_mul_add_is_the_reference(dtype):
    """chain_mul_add is the port's convf (and the compiled reference's, where built) bit for bit, on every format, with
    a scale, an offset and a zero tap; chain_fma stays within 1 ULP of it on non-negative pels."""
    src = image(41, 9, 2, dtype, 3)
    mask, scale = random_mask(9, 5, 4)
    mask[2, 3] = 0.0
    got = chain_mul_add(src, mask, scale, -2.5)
    same_bits(got, reference(src, mask, scale, -2.5), "port")
    if helpers.have_ref():
        same_bits(got, Ref.run_mask("conv", src, mask, scale, -2.5, "precision=float"), "reference")
    ys, es = sample_points(src.shape, 1, n_random=60)
    assert ulp_distance(chain_fma(src, mask, scale, -2.5, ys, es), got.reshape(9, -1)[ys, es]) <= 1


# ---------------------------------------------------------------- B. one-sign masks on non-negative data

@gpu
@pytest.mark.parametrize("width", [511, 512, 2047, 2048, 2049, 2048 + 70])
def test_lds_kernel_default_mode(width, device):
    """convf_rows_lds<TIN, 4, true>: one band, 8- and 16-bit pels, masks 8 .. 64 wide and 4 or more high, images 512
    or more wide.  Widths round the 2048 columns of a block (511: not this kernel, the grouped one takes it); heights
    round the R = 4 rows of a block; every mask width whose staged window differs (8 .. 64: 1 .. 8 groups of taps, 64
    with the `extra` lanes' share at its largest); mask heights 4 and 9; all four formats.  Beside them what the
    kernel must NOT take: 7 wide (no fused kernel: default == exact), 65 wide and 3 high (the grouped kernel: still
    chain_fma's bits).
    Vacuity, asserted per width: chain_fma and chain_mul_add store different floats on at least one sampled output.
    Observed: 1 (the aimed output) at every width; 0 on the Gaussian masks."""
    differ = 0
    for mw, mh in ((8, 4), (9, 9), (16, 4), (17, 4), (31, 9), (64, 4)):
        mask, scale = gauss_mask(mw, mh)
        differ += check_conv(image(width, 5, 1, np.uint16, 200 + mw), mask, scale, 0.0, mw, "lds")
    for height in (1, 3, 4, 13):
        mask, scale = gauss_mask(17, 9)
        differ += check_conv(image(width, height, 1, np.uint8, 210 + height), mask, scale, 0.0, height, "lds heights")
    for dtype in (np.int8, np.int16):
        mask, scale = gauss_mask(9, 4)
        differ += check_conv(image(width, 5, 1, dtype, 220), mask, scale, 0.0, 3, "lds formats")
    differ += check_aimed(image(width, 13, 1, np.uint16, 230), 16, 4, 231, (6, width // 2 + 1), "lds")
    mask, scale = gauss_mask(7, 4)
    check_conv(image(width, 5, 1, np.uint16, 240), mask, scale, 0.0, 5, "7 wide", fused=False)
    mask, scale = gauss_mask(65, 4)
    differ += check_conv(image(width, 5, 1, np.uint16, 241), mask, scale, 0.0, 6, "65 wide")
    mask, scale = gauss_mask(9, 3)
    differ += check_conv(image(width, 5, 1, np.uint16, 242), mask, scale, 0.0, 7, "3 high")
    print("lds, width %d: the chains part on %d sampled outputs" % (width, differ))
    assert differ >= 1


@gpu
@pytest.mark.parametrize("bands", [1, 2, 3, 4, 5])
def test_grouped_kernel_default_mode(bands, device, monkeypatch):
    """convf_grouped<TIN, float, EPP, true> with the LDS kernel switched off: bands 1 .. 5 reach EPP 1, 0, 3, 4 and 0.
    Widths 5 (every tap clamped), 37, 255 / 256 / 257 (round a wave's 32 tiles of 8) and 1030 (more than one block of
    2048 elements from 2 bands on; one band gets 2049 columns for its seam); mask widths 8 .. 65 (1 .. 9 groups of
    taps: an odd and an even number of loop trips, the last group whole and partial) with heights 1, 3, 4 and 9; all
    six formats; 7 wide: no fused kernel, default == exact.
    Vacuity, asserted per band count: the chains store different floats on at least one sampled output.
    Observed: 1 (the aimed output) for every band count; 0 on the Gaussian masks."""
    monkeypatch.setenv("VIPS_HIP_NO_LDS_CONV", "1")
    differ = 0
    widths = (5, 37, 255, 256, 257, 1030) + ((2049,) if bands == 1 else ())
    for width in widths:
        mask, scale = gauss_mask(9, 3)
        differ += check_conv(image(width, 4, bands, np.uint16, 300 + width), mask, scale, 0.0, width, "grouped widths")
    for mw, mh in ((8, 1), (16, 3), (17, 4), (31, 9), (64, 1), (65, 3)):
        mask, scale = gauss_mask(mw, mh)
        differ += check_conv(image(257, 5, bands, np.uint8, 310 + mw), mask, scale, 0.0, mw, "grouped masks")
    for dtype in (np.int8, np.int16, np.uint32, np.int32):
        mask, scale = gauss_mask(8, 3)
        differ += check_conv(image(1030, 3, bands, dtype, 320), mask, scale, 0.0, 4, "grouped formats")
    differ += check_aimed(image(1030, 5, bands, np.uint16, 330), 16, 4, 331, (2, 515 * bands + bands - 1), "grouped")
    mask, scale = gauss_mask(7, 3)
    check_conv(image(257, 5, bands, np.uint16, 340), mask, scale, 0.0, 5, "7 wide", fused=False)
    print("grouped, %d bands: the chains part on %d sampled outputs" % (bands, differ))
    assert differ >= 1


@gpu
@pytest.mark.parametrize("bands", [1, 3])
def test_no_grouped_kernel_nothing_fused(bands, device, monkeypatch):
    """$VIPS_HIP_NO_GROUPED_CONV keeps both fused kernels out: the default mode then gives the reference's bits, on an
    image either of them would have taken."""
    monkeypatch.setenv("VIPS_HIP_NO_GROUPED_CONV", "1")
    mask, scale = gauss_mask(9, 9)
    check_conv(image(530, 6, bands, np.uint16, 350), mask, scale, 0.0, 1, "no grouped kernel", fused=False)
    mask, scale = random_mask(16, 4, 351)
    check_conv(image(530, 6, bands, np.uint8, 352), mask, scale, 3.25, 1, "no grouped kernel", fused=False)


def region_conv(src, rect, mask, scale, offset):
    """vips_hip_conv_gen of the out rect (left, top, w, h) from a window of `src` that only just holds the halo."""
    H, W, bands = src.shape
    mh, mw = mask.shape
    left, top, w, h = rect
    x0, y0 = max(left - mw // 2, 0), max(top - mh // 2, 0)
    x1, y1 = min(left + w - 1 - mw // 2 + mw, W), min(top + h - 1 - mh // 2 + mh, H)
    plan = lib.vips_hip_conv_new(mask.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), mw, mh, scale, offset,
                                 libvips_amd.PRECISIONS["float"])
    assert plan
    try:
        win = Image.new_from_array(np.ascontiguousarray(src[y0:y1, x0:x1]))
        rin = win.region()
        rin.left, rin.top, rin.im_width, rin.im_height = x0, y0, W, H
        out = Image.new_from_array(np.zeros((h, w, bands), np.float32))
        rout = out.region()
        rout.left, rout.top, rout.im_width, rout.im_height = left, top, W, H
        _ffi.check(lib.vips_hip_conv_gen(plan, ctypes.byref(rin), ctypes.byref(rout)))
        return out.numpy(), (x0, rin.stride)
    finally:
        lib.vips_hip_conv_free(plan)


@gpu
@pytest.mark.parametrize("case", [(np.uint8, 1, 90), (np.uint8, 3, 90), (np.uint16, 2, 90), (np.uint8, 1, 700)],
                         ids=lambda c: "%s-%d-%d" % (np.dtype(c[0]).name, c[1], c[2]))
def test_region_form_default_mode(case, device):
    """vips_hip_conv_gen on a window that only just holds the halo, its left edge and its stride no multiples of 4: the
    INTERIOR = false rows of convf_grouped_rows away from the image's edges (EPP 1, 3 and the any-bands variant), and
    the LDS kernel's window clamp (the 700-wide case: an out rect of 531 columns).  Rects inside the image and on its
    edges, against the same rect of the whole image's reference and of chain_fma.
    Vacuity, asserted: the chains store different floats on at least one sampled output (the first rect holds an aimed
    one).  Observed: 1 in each of the four cases."""
    dtype, bands, W = case
    H = 40
    src = image(W, H, bands, dtype, 360 + bands)
    mask, scale = random_mask(9, 5, 361)
    rects = ((33, 5, 531, 6), (0, 0, 523, 3)) if W == 700 else ((21, 15, 43, 9), (0, 0, 19, 6), (67, 31, 23, 9), (3, 33, 85, 7))
    left, top, w, h = rects[0]
    offset, target = aimed_offset(src, mask, scale, -3.5, top + h // 2, left * bands, count=w * bands)
    want = reference(src, mask, scale, offset)
    sums = chain_mul_add(src, mask, scale, offset, store=False)
    same_bits(sums.astype(np.float32), want, "chain_mul_add against the port")
    parted = 0
    for k, rect in enumerate(rects):
        left, top, w, h = rect
        want_rect = np.ascontiguousarray(want[top:top + h, left:left + w])
        exact, _ = region_conv(src, rect, mask, scale, offset)
        same_bits(exact, want_rect, "exact mode, region %r" % (rect,))
        with default_mode():
            fast, (x0, stride) = region_conv(src, rect, mask, scale, offset)
        if k == 0:
            # (a ushort pel of two bands is four bytes: every stride is a multiple of 4)
            assert x0 % 4 and (stride % 4 or bands * src.itemsize == 4), (x0, stride)
        assert ulp_distance(fast, want_rect) <= 1, rect  # tolerance: 1 ULP (BASELINE.json north_star)
        extra = [(y - top, e - left * bands) for y, e in near_boundaries(sums, 32)
                 if top <= y < top + h and left * bands <= e < (left + w) * bands]
        ys, es = sample_points((h, w, bands), 370 + k, extra=extra, n_random=100)
        fm = chain_fma(src, mask, scale, offset, ys + top, es + left * bands)
        got = fast.reshape(h, -1)[ys, es]
        bad = np.nonzero(bits(got) != bits(fm))[0]
        assert len(bad) == 0, "region %r: %d of %d sampled differ from chain_fma, first at (y %d, e %d)" % (
            rect, len(bad), len(ys), ys[bad[0]], es[bad[0]])
        parted += int((bits(fm) != bits(want_rect.reshape(h, -1)[ys, es])).sum())
    print("region form %s: the chains part on %d sampled outputs" % (case, parted))
    assert parted >= 1


# ---------------------------------------------------------------- C. masks whose taps differ in sign

def gauss_row(sigma, n):
    x = np.arange(n) - n // 2
    g = np.exp(-x * x / (2.0 * sigma * sigma))
    return g / g.sum()


def mixed_masks():
    """name -> mask (scale 1, offset 0): a Gaussian outer a derivative of Gaussian, differences of Gaussians (their
    coefficients sum to nearly nothing: on a flat image only the roundings are left)."""
    g9, g15 = gauss_row(1.5, 9), gauss_row(2.5, 15)
    d9 = -(np.arange(9) - 4) * g9
    return {
        "gauss_x_dgauss_9x9": np.ascontiguousarray(np.outer(g9, d9)),
        "dog_9x9": np.ascontiguousarray(np.outer(g9, g9) - np.outer(gauss_row(2.5, 9), gauss_row(2.5, 9))),
        "dog_1x9": np.ascontiguousarray((g9 - gauss_row(2.5, 9))[None, :]),
        "dog_15x15": np.ascontiguousarray(np.outer(g15, g15) - np.outer(gauss_row(4.0, 15), gauss_row(4.0, 15))),
    }


def mixed_images(w, h, bands, dtype):
    flat = 40000 if np.dtype(dtype) == np.uint16 else 200
    top = 65535 if np.dtype(dtype) == np.uint16 else 255
    ramp = (np.arange(w)[None, :, None] * (top // w) + np.arange(bands)[None, None, :]) + np.zeros((h, 1, 1), int)
    return {"flat": np.full((h, w, bands), flat, dtype), "ramp": np.ascontiguousarray(ramp.astype(dtype)),
            "noise": image(w, h, bands, dtype, 400 + bands)}


def chains_apart(src, mask, n=24):
    """The largest ULP distance between what the two chains store, over a few outputs of a small image."""
    ys, es = sample_points(src.shape, 9, n_random=n)
    keep = np.arange(len(ys))[:: max(1, len(ys) // (2 * n))]
    ys, es = ys[keep], es[keep]
    fm = chain_fma(src, mask, 1.0, 0.0, ys, es)
    ma = chain_mul_add(src, mask, 1.0, 0.0).reshape(src.shape[0], -1)[ys, es]
    return ulp_distance(fm, ma)


@gpu
@pytest.mark.parametrize("lds", [True, False], ids=["lds", "no-lds"])
@pytest.mark.parametrize("bands", [1, 3])
def test_mixed_sign_masks_take_the_exact_arithmetic(bands, lds, device, monkeypatch):
    """conv.hip follows convsep_stream.hip's rule: a mask whose non-zero taps differ in sign can cancel, a cancelling
    sum has no 1 ULP bound, so it takes the FUSED = false kernels whatever the mode -- the default mode gives the
    reference's bits.  Four masks x flat / ramp / noise images x ushort and uchar, on an image the LDS kernel takes (one
    band, 530 wide) and with that kernel off.
    Vacuity, asserted per mask and format: on the flat image the two host chains store floats MORE than 1 ULP apart, so
    a kernel that fused these masks would be caught.  Observed (largest distance on the flat image, ushort / uchar):
    gauss_x_dgauss_9x9 1 428 524 304 / 5 694 464, dog_9x9 2 058 624 / 10 141 696, dog_1x9 7 081 984 / 1 179 648,
    dog_15x15 949 304 / 102 656 -- the same for one and three bands; on noise the chains store the same floats."""
    if not lds:
        monkeypatch.setenv("VIPS_HIP_NO_LDS_CONV", "1")
    for dtype in (np.uint16, np.uint8):
        images = mixed_images(530, 6, bands, dtype)
        for name, mask in sorted(mixed_masks().items()):
            assert (mask < 0).any() and (mask > 0).any()
            assert chains_apart(images["flat"][:, :40], mask) > 1, name
            for kind, src in sorted(images.items()):
                want = reference(src, mask, 1.0, 0.0)
                with default_mode():
                    got = run_conv(src, mask, 1.0, 0.0)
                same_bits(got, want, "default mode, %s on %s %s x%d" % (name, kind, np.dtype(dtype).name, bands))
                same_bits(run_conv(src, mask, 1.0, 0.0), want, "exact mode, %s on %s" % (name, kind))


@gpu
@pytest.mark.parametrize("precision,scale,offset", [("integer", 19.0, 3.0), ("float", 18.5, -0.75)])
def test_convsep_stream_mixed_sign_guard(precision, scale, offset, device):
    """convsep_stream.hip's own guard (it clears `fast` for a mask whose taps differ in sign): a float image, the mask
    of test_fused_convsep_float_offsets_and_nonfinite, default mode: the port's bits, and by the streaming kernel."""
    src = helpers.lcg_image(333, 40, 3, np.float32, 68)
    mask = np.array([[-1.0, 2.0, 5.0, 7.0, 5.0, 3.0, -2.0]])
    want = PortCC.convsep(src, mask, scale, offset, precision)
    with default_mode(), gated() as g:
        got = Image.new_from_array(src).convsep(mask, scale=scale, offset=offset, precision=precision).numpy()
    assert any(k.startswith("convsep_stream") for k in g.report), g.report
    same_bits(got, want, "convsep %s" % precision)


# ---------------------------------------------------------------- D. signed formats

@gpu
@pytest.mark.parametrize("dtype", [np.int16, np.int32], ids=lambda d: np.dtype(d).name)
def test_signed_formats_non_negative_pels(dtype, device):
    """short (the LDS kernel: one band, 530 wide; and the grouped one: three bands) and int (the grouped kernel) with
    non-negative pels: inside the header's bound, so (a) and (b) both.
    Vacuity, asserted: the chains store different floats on at least one sampled output of the aimed mask.
    Observed: 1 for both formats."""
    mask, scale = gauss_mask(17, 5)
    check_conv(image(530, 6, 1, dtype, 500), mask, scale, 0.0, 1, "signed format")
    check_conv(image(261, 5, 3, dtype, 501), mask, scale, 0.0, 2, "signed format")
    assert check_aimed(image(530, 6, 1, dtype, 502), 16, 4, 503, (3, 266), "signed format") >= 1


@gpu
@pytest.mark.parametrize("dtype", [np.int8, np.int16, np.int32], ids=lambda d: np.dtype(d).name)
def test_signed_formats_pels_of_both_signs(dtype, device):
    """Pels of both signs under a one-sign mask can cancel like taps of both signs under one-sign pels: the header's
    1 ULP bound does not cover them (and the mode's arithmetic is the same), so only (b): chain_fma's bits.  The
    exact mode still gives the reference's."""
    mask, scale = gauss_mask(17, 5)
    src = image(530, 6, 1, dtype, 510, both_signs=True)
    assert (src < 0).any() and (src > 0).any()
    check_conv(src, mask, scale, 0.0, 1, "both signs", contract=False)
    check_conv(image(261, 5, 3, dtype, 511, both_signs=True), mask, scale, 0.0, 2, "both signs", contract=False)
    # a wide Gaussian over columns of +v and -v: the sum nearly cancels; still chain_fma's bits
    stripes = np.where(np.arange(530) % 2 == 0, 100, -100).astype(dtype)[None, :, None] + np.zeros((6, 1, 1), dtype)
    check_conv(np.ascontiguousarray(stripes), mask, scale, 0.0, 3, "stripes", contract=False)


# ---------------------------------------------------------------- E. what stands on the blur

# (name, input format, bands, sigma, precision, the blur must differ between the modes)
CANNY_CASES = [("float-1", np.float32, 1, 1.4, "float", False), ("float-3", np.float32, 3, 1.4, "float", False),
               ("float-1-integer", np.float32, 1, 2.0, "integer", True), ("float-3-integer", np.float32, 3, 2.0, "integer", True),
               ("ushort", np.uint16, 1, 1.4, "float", False), ("uchar-1.4", np.uint8, 1, 1.4, "float", False),
               ("uchar-3.0", np.uint8, 1, 3.0, "float", False)]


def canny_input(dtype, bands, width, height, precision):
    if np.dtype(dtype) == np.uint8:
        return noise(width, height, bands, np.uint8, 151 + bands)
    if precision == "integer":  # (a cast uchar image: see test_canny_default_mode)
        return noise(width, height, bands, np.uint8, 151 + bands).astype(dtype)
    return ranged(width, height, bands, dtype, 161 + bands)


@gpu
@needs_ref
@pytest.mark.parametrize("case", CANNY_CASES, ids=lambda c: c[0])
def test_canny_default_mode(case, device):
    """vips_hip_canny promises the reference's bits whenever canny_marginal() == 0, and a decision hangs on its blur
    (the gradient is a difference of neighbours, thinning keeps or zeroes a pel): it runs its blur in the exact
    arithmetic whatever the mode (ScopedExactFloat), and hands the mode back as it found it.  With the default
    precision (float) a float input goes through convsep_stream (MODE 3 in the default mode), uchar and ushort
    through convf_grouped on the first pass -- sigma 3.0 gives the uchar case a mask 8 or more wide.  Sizes round the
    canny kernel's tile, and 131 x 37.
    Vacuity: the two modes' blurs (Image.gaussblur of the same image) must differ somewhere, or a canny that blurred in
    the caller's mode would pass as well.  At these sizes they do NOT differ for any of the default-precision inputs
    (observed: 0 of 12 838 elements a band; 0 of 2 000 000 on each of three 2000 x 1000 float noise images): one
    rounding per tap instead of two moves a float only where the double sum lies within a few units of 2^-53 of a
    rounding boundary.  convsep_stream.hip's head says where that is common: integer taps on pels that are short
    binary fractions put sum / scale exactly ON a boundary.  So the float input also runs as a cast uchar image with
    precision integer and sigma 2.0 (taps 6 12 18 20 18 12 6, scale 92), and there the assertion holds.  Observed:
    the blurs differ in 33 of 12 838 elements (one band) and in 102 of 38 514 (three bands) over the five sizes."""
    _, dtype, bands, sigma, precision, must_differ = case
    tw, th = canny_tile()
    blur_differs = 0
    for width, height in ((tw - 1, th + 1), (tw, th), (tw + 1, th - 1), (2 * tw + 5, 2 * th + 5), (131, 37)):
        src = canny_input(dtype, bands, width, height, precision)
        exact_blur = Image.new_from_array(src).gaussblur(sigma, precision=precision).numpy()
        with default_mode():
            fast_blur = Image.new_from_array(src).gaussblur(sigma, precision=precision).numpy()
            check_canny(src, sigma, precision, "default mode")
            assert lib.vips_hip_get_exact_float() == 0  # the scope does not leak into the caller
        assert ulp_distance(fast_blur, exact_blur) <= 1  # tolerance: 1 ULP (BASELINE.json north_star)
        blur_differs += int((bits(fast_blur) != bits(exact_blur)).sum())
    print("canny %s: the two modes' blurs differ in %d elements" % (case[0], blur_differs))
    if must_differ:
        assert blur_differs > 0


COMPASS_POSITIVE, COMPASS_SCALE = random_mask(9, 9, 600)


@gpu
@needs_ref
@pytest.mark.parametrize("combine", ["max", "sum"])
@pytest.mark.parametrize("bands", [1, 3])
def test_compass_default_mode(bands, combine, device):
    """vips_compass with precision float is continuous in its convolutions (abs, then max or sum): no decision, so it
    runs in the caller's mode and the header's bound is what it promises.  A 9 x 9 positive fractional mask, times 4,
    ushort: default mode within 1 ULP of the reference, exact mode its bits; a 9 x 9 mask of both signs (the
    difference of Gaussians of section C; the left half of the image is flat, which is where a fused sum would show):
    the default mode gives the exact mode's bits (the rule of conv.hip)."""
    src = image(150, 20, bands, np.uint16, 610 + bands)
    src[:, :75] = 40000
    mixed_mask = mixed_masks()["dog_9x9"]
    args = "times=4,angle=d90,combine=%s,precision=float" % combine

    def run(mask, scale):
        return Image.new_from_array(src).compass(mask, times=4, angle="d90", combine=combine, precision="float",
                                                 scale=scale).numpy()

    want = Ref.run_mask("compass", src, COMPASS_POSITIVE, COMPASS_SCALE, 0.0, args=args)
    same(run(COMPASS_POSITIVE, COMPASS_SCALE), want, "compass, exact mode")
    with default_mode():
        fast = run(COMPASS_POSITIVE, COMPASS_SCALE)
        mixed = run(mixed_mask, 1.0)
    assert fast.dtype == want.dtype == np.float32 and fast.shape == want.shape
    assert ulp_distance(fast, want) <= 1  # tolerance: 1 ULP (BASELINE.json north_star)
    assert (mixed_mask < 0).any() and (mixed_mask > 0).any()
    same(mixed, run(mixed_mask, 1.0), "compass, mask of both signs: default mode against exact")
    same(mixed, Ref.run_mask("compass", src, mixed_mask, 1.0, 0.0, args=args), "compass, mask of both signs")


@gpu
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16], ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("sigma", [3.0, 8.0])
def test_gaussblur_integer_formats_default_mode(sigma, dtype, device):
    """gaussblur with precision float on uchar / ushort: the first pass is an integer image through convf_grouped
    (fused in the default mode), the second a float image with a mask one wide (never fused).  Within 1 ULP of the
    port, 1 and 3 bands; the exact mode its bits."""
    for bands in (1, 3):
        src = image(300, 20, bands, dtype, 620 + bands)
        want = PortCC.gaussblur(src, sigma, precision="float")
        same_bits(Image.new_from_array(src).gaussblur(sigma, precision="float").numpy(), want, "exact mode")
        with default_mode():
            fast = Image.new_from_array(src).gaussblur(sigma, precision="float").numpy()
        assert fast.dtype == np.float32 and fast.shape == want.shape
        assert ulp_distance(fast, want) <= 1  # tolerance: 1 ULP (BASELINE.json north_star)


@gpu
def test_smartcrop_same_crop_in_both_modes(device):
    """The attention search asks for the exact arithmetic itself (smartcrop.cpp): the same crop in both modes, and the
    caller's mode untouched."""
    from tests.test_smartcrop_gpu import new_image, scene

    src = scene(200, 150, 3, 5, 150, 100, 25)
    exact, exact_opts = new_image(src).smartcrop(64, 64, interesting="attention", with_options=True)
    with default_mode():
        fast, fast_opts = new_image(src).smartcrop(64, 64, interesting="attention", with_options=True)
        assert lib.vips_hip_get_exact_float() == 0
    assert fast_opts == exact_opts
    assert np.array_equal(fast.numpy(), exact.numpy())


# ---------------------------------------------------------------- F. the mode itself (host only)

def test_mode_set_and_get():
    before = lib.vips_hip_get_exact_float()
    try:
        lib.vips_hip_set_exact_float(0)
        assert lib.vips_hip_get_exact_float() == 0
        lib.vips_hip_set_exact_float(1)
        assert lib.vips_hip_get_exact_float() == 1
        lib.vips_hip_set_exact_float(5)  # (any non-zero value enables)
        assert lib.vips_hip_get_exact_float() == 1
    finally:
        lib.vips_hip_set_exact_float(before)


MODE_CHILD = r"""
import os, sys
sys.path.insert(0, %r)
from libvips_amd import lib
first = lib.vips_hip_get_exact_float()
os.environ["VIPS_HIP_EXACT_FLOAT"] = "0" if first else "1"  # too late: the first use decided
second = lib.vips_hip_get_exact_float()
lib.vips_hip_set_exact_float(0 if first else 1)  # a call always wins
print("MODE", first, second, lib.vips_hip_get_exact_float())
"""


@pytest.mark.parametrize("value,want", [(None, 0), ("0", 0), ("1", 1), ("7", 1), ("", 0)])
def test_mode_environment_at_first_use(value, want):
    """$VIPS_HIP_EXACT_FLOAT is read once, at the first use, in a process that never set the mode: unset, empty or 0
    leave the default mode, any other number selects the exact one; the variable is not read again;
    vips_hip_set_exact_float overrides it."""
    env = {k: v for k, v in os.environ.items() if k != "VIPS_HIP_EXACT_FLOAT"}
    if value is not None:
        env["VIPS_HIP_EXACT_FLOAT"] = value
    proc = subprocess.run([sys.executable, "-c", MODE_CHILD % helpers.ROOT], stdout=subprocess.PIPE,
                          stderr=subprocess.STDOUT, text=True, env=env, cwd=helpers.ROOT, timeout=120)
    assert proc.returncode == 0, proc.stdout[-2000:]
    assert "MODE %d %d %d" % (want, want, 1 - want) in proc.stdout, proc.stdout[-2000:]
