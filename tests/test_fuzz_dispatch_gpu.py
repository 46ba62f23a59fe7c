"""GPU: a seeded fuzz over the DISPATCH GUARDS of the streaming and matrix-core kernels of rounds 4 and 5
(reduceh_u8_packed, shrinkh_u8_stream, conv_u8 / conv_u8_mfma, conv_u16, reducev_u8_stream, reduce_band,
resample16): sizes round the dword / quad / 16-byte / strip / segment boundaries, 1 .. 4 bands, widths whose
rows are NOT whole dwords (the fall-back must be taken and still match), fractional and integer factors, masks
round the coefficient limits; the colour kind walks the guard of the 4-pixels-per-lane colour route kernels (bands,
width & 3, pointer and stride alignment in region form) over the pairs of vips_colourspace.  Whatever kernel the library picks, the result must equal the reference's (the
compiled reference when present, else the port) bit for bit; the report must name a kernel.  The host-fiber fuzz
of round 4 (tools/fuzz_emul.py) cannot see what only the device does: waitcnt, compiler traps, the LDS-DMA."""
import random

import numpy as np
import pytest

import libvips_amd
from libvips_amd import Image
from tests import helpers

pytestmark = pytest.mark.gpu

EDGES = [4, 8, 12, 16, 28, 32, 36, 60, 64, 68, 124, 128, 132, 252, 256, 260, 508, 512, 516, 1020, 1024, 1028]


def _size(rng, lo=8, hi=1400):
    # a boundary, a boundary +- a little, or anything
    r = rng.random()
    if r < 0.4:
        return max(lo, rng.choice(EDGES) + rng.choice([-3, -2, -1, 0, 0, 1, 2, 3]))
    if r < 0.6:
        return max(lo, rng.choice(EDGES) * rng.choice([1, 2, 3]))
    return rng.randrange(lo, hi)


def _reference(chain, src, port_call):
    if helpers.have_ref():
        return helpers.Ref.run_chain(chain, src)
    return port_call()


# ---- the colour kind: the guard of the 4-pixels-per-lane route kernels (bands, width & 3, the alignment of the row
# pointers and strides) over the supported pairs of vips_colourspace

COLOUR_SPACES = ["b-w", "grey16", "rgb16", "srgb", "scrgb", "xyz", "lab", "labs"]
COLOUR_PAIRS = [(a, b) for a in COLOUR_SPACES for b in COLOUR_SPACES
                if not (a in ("b-w", "grey16") and b in ("xyz", "lab", "labs"))]
assert len(COLOUR_PAIRS) == 58
# (the routes with kernels of their own are drawn more often: two of them are the only way to a compiled-in route)
COLOUR_FAST = [("srgb", "lab"), ("srgb", "labs"), ("labs", "srgb"), ("lab", "srgb")]
COLOUR_STEP_NUMBERS = {"sRGB2scRGB": 0, "scRGB2XYZ": 1, "XYZ2Lab": 2, "Lab2XYZ": 3, "XYZ2scRGB": 4, "scRGB2sRGB": 5,
                       "Lab2LabS": 7, "LabS2Lab": 8}
COLOUR_GATES = ("colour_lab_quad", "colour_lab_lds", "colour_route_x4_static", "colour_route_x4", "colour_route")
COLOUR_OUT = {"srgb": np.uint8, "labs": np.int16, "scrgb": np.float32, "xyz": np.float32, "lab": np.float32}


class _Pixels(object):
    def __init__(self, array):
        self.array = array

    def numpy(self):
        return self.array


def _colour_source(rng, a, w, h, extra, seed):
    from tests import colour_domains as dom

    if a in ("b-w", "grey16"):
        return helpers.lcg_image(w, h, 1 + extra, np.uint8 if a == "b-w" else np.uint16, seed)
    fmt = "u8"
    if a == "srgb" and rng.random() < 0.4:
        fmt = "f32"
    return dom.layout_input(a, fmt, w, h, 3 + extra, seed)


def _colour_reference(src, a, b):
    if helpers.have_ref():
        return helpers.Ref.run("colourspace", src, "space=" + b, helpers.INTERP[a])
    return helpers.PortCC.colourspace(src, b, a)


def _colour_case(rng, seed):
    import ctypes

    from libvips_amd import _ffi

    region = rng.random() < 1.0 / 3
    if region or not helpers.have_ref():
        # region form takes the step list: the pairs with a fused 3-band route (the port's routes, when it referees)
        a, b = rng.choice(sorted(helpers.PortCC._ROUTES) + 3 * COLOUR_FAST)
    else:
        # (a space to itself is a copy, or a plain cast: no colour kernel, nothing for the report to name)
        a, b = rng.choice([p for p in COLOUR_PAIRS if p[0] != p[1]] + 3 * COLOUR_FAST)
    if not region:
        w, h = _size(rng, 4), _size(rng, 4, 300)
        extra = rng.choice([0, 0, 0, 1, 2])
        src = _colour_source(rng, a, w, h, extra, seed)
        if src.dtype == np.float32 and a == "srgb" and b == "rgb16":
            src = src.clip(0, 255).astype(np.uint8)  # (a shift cast of a float image is refused)
        im = Image.new_from_array(src, interpretation=a)
        return ("colour", a, b, w, h, src.shape[2], src.dtype.name), lambda: im.colourspace(b), \
            lambda: _colour_reference(src, a, b)
    # a window of an image as the input region, a rectangle of that window as the output: aligned or not
    full_w, full_h = _size(rng, 24), _size(rng, 8, 200)
    src = _colour_source(rng, a, full_w, full_h, 0, seed)
    aligned = rng.random() < 0.5
    pick = (lambda hi: 4 * rng.randrange(0, hi // 4 + 1)) if aligned else (lambda hi: rng.randrange(0, hi + 1))
    x0 = pick(full_w // 4)
    ww = max(4, full_w - x0 - pick(full_w // 4))
    left = x0 + pick(ww // 3)
    w = max(1, x0 + ww - left - pick(ww // 3))
    if aligned:
        ww, w = max(4, ww & ~3), max(4, w & ~3)
        w = min(w, (x0 + ww - left) & ~3)
    y0 = rng.randrange(0, full_h // 3 + 1)
    wh = full_h - y0 - rng.randrange(0, full_h // 3 + 1)
    top = y0 + rng.randrange(0, wh // 2 + 1)
    h = max(1, y0 + wh - top - rng.randrange(0, wh // 3 + 1))
    steps = [COLOUR_STEP_NUMBERS[s] for s in helpers.PortCC._ROUTES[(a, b)]]

    def call():
        win = Image.new_from_array(np.ascontiguousarray(src[y0:y0 + wh, x0:x0 + ww]))
        rin = win.region()
        rin.left, rin.top, rin.im_width, rin.im_height = x0, y0, full_w, full_h
        out = Image.new_from_array(np.zeros((h, w, 3), COLOUR_OUT[b]))
        rout = out.region()
        rout.left, rout.top, rout.im_width, rout.im_height = left, top, full_w, full_h
        arr = (ctypes.c_int * len(steps))(*steps)
        _ffi.check(_ffi.lib.vips_hip_colour_route_gen(arr, len(steps), ctypes.c_double(1.0), ctypes.byref(rin),
                                                      ctypes.byref(rout)))
        return _Pixels(out.numpy())
    return ("colour-region", a, b, full_w, full_h, (x0, y0, ww, wh), (left, top, w, h), src.dtype.name), call, \
        lambda: np.ascontiguousarray(_colour_reference(src, a, b)[top:top + h, left:left + w])


def _case(rng, kind):
    seed = rng.randrange(1 << 30)
    bands = rng.choice([1, 2, 3, 3, 4])
    if kind == "reduce":
        w, h = _size(rng, 16), _size(rng, 16)
        dt = rng.choice([np.uint8, np.uint8, np.uint16])
        src = helpers.lcg_image(w, h, bands, dt, seed)
        shrink = rng.choice([2.0, 4.0, 8.0, 1.3 + 9 * rng.random(), 2.0 + 6 * rng.random()])
        shrink = round(shrink, 3)
        kernel = rng.choice(["lanczos3", "lanczos3", "lanczos2", "cubic", "mitchell", "linear"])
        axis = rng.choice(["reduceh", "reducev", "reduce"])
        im = Image.new_from_array(src)
        if axis == "reduce":
            call = lambda: im.reduce(shrink, shrink, kernel=kernel)
            chain = "reduce:hshrink=%r,vshrink=%r,kernel=%s" % (shrink, shrink, kernel)
            port = lambda: helpers.Port.reduce(src, shrink, shrink, kernel)
        elif axis == "reduceh":
            call = lambda: im.reduceh(shrink, kernel=kernel)
            chain = "reduceh:hshrink=%r,kernel=%s" % (shrink, kernel)
            port = lambda: helpers.Port.reduce(src, shrink, 1.0, kernel)
        else:
            call = lambda: im.reducev(shrink, kernel=kernel)
            chain = "reducev:vshrink=%r,kernel=%s" % (shrink, kernel)
            port = lambda: helpers.Port.reduce(src, 1.0, shrink, kernel)
        return (kind, axis, w, h, bands, dt.__name__, shrink, kernel), call, lambda: _reference(chain, src, port)
    if kind == "shrink":
        w, h = _size(rng, 16), _size(rng, 16)
        dt = rng.choice([np.uint8, np.uint8, np.uint16])
        src = helpers.lcg_image(w, h, bands, dt, seed)
        hs, vs = rng.choice([1, 2, 3, 4, 5, 8, 12]), rng.choice([1, 2, 3, 4, 8])
        im = Image.new_from_array(src)
        chain = "shrink:hshrink=%d,vshrink=%d" % (hs, vs)
        return (kind, w, h, bands, dt.__name__, hs, vs), lambda: im.shrink(hs, vs), \
            lambda: _reference(chain, src, lambda: helpers.Port.shrink(src, hs, vs))
    if kind == "blur":
        w, h = _size(rng, 8), _size(rng, 8)
        src = helpers.lcg_image(w, h, bands, np.uint8, seed)
        sigma = rng.choice([0.8, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, 8.0])
        im = Image.new_from_array(src)
        return (kind, w, h, bands, sigma), lambda: im.gaussblur(sigma), \
            lambda: _reference("gaussblur:sigma=%r" % sigma, src, lambda: helpers.PortCC.gaussblur(src, sigma))
    if kind == "convsep":
        w, h = _size(rng, 8), _size(rng, 8)
        src = helpers.lcg_image(w, h, bands, np.uint8, seed)
        n = rng.choice([3, 5, 7, 9, 13, 17, 25, 33])
        top = rng.choice([9, 127, 128, 300, 2047])
        mask = [rng.randrange(-top // 4, top + 1) for _ in range(n)]
        mask[n // 2] = top
        scale = max(1, sum(mask))
        im = Image.new_from_array(src)

        def ref():
            m = np.asarray(mask, dtype=np.float64)
            if helpers.have_ref():
                return helpers.Ref.run_mask("convsep", src, m[None, :], scale, 0.0, "precision=integer")
            return helpers.PortCC.convsep(src, m, scale=scale, precision="integer")
        return (kind, w, h, bands, mask, scale), lambda: im.convsep(mask, scale=scale, precision="integer"), ref
    if kind == "resize":
        # round 6: vips_resize across the SIZE threshold that picks the chain of band kernels
        # (images of 8 MB and more, tools/band_threshold.py) or the one-kernel chain: images of 7 .. 9 MB
        bands = rng.choice([3, 3, 4, 1])
        target = rng.choice([7.0, 7.9, 8.0, 8.1, 9.0]) * (1 << 20)
        w = rng.randrange(900, 2600)
        w -= (w * bands) % 4 if rng.random() < 0.7 else 0  # (mostly rows of whole dwords: the streaming kernels' case)
        h = max(64, int(target / (w * bands)) + rng.choice([-1, 0, 1]))
        src = helpers.lcg_image(w, h, bands, np.uint8, seed)
        scale = round(rng.choice([0.125, 0.25, 0.05 + 0.4 * rng.random(), 0.05 + 0.4 * rng.random()]), 4)
        im = Image.new_from_array(src)
        return (kind, w, h, bands, scale), lambda: im.resize(scale), \
            lambda: _reference("resize:scale=%r" % scale, src, lambda: helpers.Port.resize(src, scale))
    if kind == "float":
        # the float streams of round 6 (resample_f32.hip) and what they decline: rows of odd element counts, images
        # too narrow, fractional factors, other kernels
        w, h = _size(rng, 16, 2200), _size(rng, 16, 600)
        bands = rng.choice([1, 3, 3, 4])
        src = (helpers.lcg_image(w, h, bands, np.uint8, seed).astype(np.float32) - 90.0) * np.float32(0.37)
        op = rng.choice(["reducev", "reduceh", "reduce", "shrinkv", "shrink"])
        im = Image.new_from_array(src)
        if op.startswith("shrink"):
            s1, s2 = rng.choice([2, 3, 4, 7, 8]), rng.choice([2, 3, 4, 8])
            if op == "shrinkv":
                return (kind, op, w, h, bands, s2), lambda: im.shrinkv(s2), \
                    lambda: _reference("shrinkv:vshrink=%d" % s2, src, lambda: helpers.Port.shrinkv(src, s2))
            return (kind, op, w, h, bands, s1, s2), lambda: im.shrink(s1, s2), \
                lambda: _reference("shrink:hshrink=%d,vshrink=%d" % (s1, s2), src, lambda: helpers.Port.shrink(src, s1, s2))
        shrink = round(rng.choice([2.0, 3.0, 4.0, 8.0, 8.0, 1.5 + 7 * rng.random()]), 3)
        kernel = rng.choice(["lanczos3", "lanczos3", "lanczos2", "cubic", "linear"])
        if op == "reducev":
            return (kind, op, w, h, bands, shrink, kernel), lambda: im.reducev(shrink, kernel=kernel), \
                lambda: _reference("reducev:vshrink=%r,kernel=%s" % (shrink, kernel), src, lambda: helpers.Port.reduce(src, 1.0, shrink, kernel))
        if op == "reduceh":
            return (kind, op, w, h, bands, shrink, kernel), lambda: im.reduceh(shrink, kernel=kernel), \
                lambda: _reference("reduceh:hshrink=%r,kernel=%s" % (shrink, kernel), src, lambda: helpers.Port.reduce(src, shrink, 1.0, kernel))
        return (kind, op, w, h, bands, shrink, kernel), lambda: im.reduce(shrink, shrink, kernel=kernel), \
            lambda: _reference("reduce:hshrink=%r,vshrink=%r,kernel=%s" % (shrink, shrink, kernel), src,
                               lambda: helpers.Port.reduce(src, shrink, shrink, kernel))
    if kind == "upsize":
        # bicubic enlargement of uchar by the column walk (upsize.hip), any bands, scales that move the window by
        # 0 / 1 input rows a step and (below 1 on one axis) by more
        w, h = _size(rng, 8, 400), _size(rng, 8, 300)
        src = helpers.lcg_image(w, h, bands, np.uint8, seed)
        hs = round(rng.choice([1.0 + 3 * rng.random(), 2.0, 2.5, 4.0]), 3)
        vs = round(rng.choice([hs, 1.0 + 3 * rng.random(), 1.0]), 3)
        im = Image.new_from_array(src)
        chain = "resize:scale=%r,vscale=%r,kernel=cubic" % (hs, vs)
        return (kind, w, h, bands, hs, vs), lambda: im.resize(hs, vscale=vs, kernel="cubic"), \
            lambda: _reference(chain, src, lambda: helpers.Port.resize(src, hs, vs, kernel="cubic"))
    if kind == "blur16":
        # ushort gaussblur across the matrix-core kernel's limits (masks of up to 33 taps: sigma 9 and more fall back)
        w, h = _size(rng, 8), _size(rng, 8)
        src = helpers.lcg_image(w, h, bands, np.uint16, seed)
        sigma = rng.choice([0.8, 1.5, 2.0, 4.0, 8.0, 8.9, 9.5, 11.0])
        im = Image.new_from_array(src)
        return (kind, w, h, bands, sigma), lambda: im.gaussblur(sigma), \
            lambda: _reference("gaussblur:sigma=%r" % sigma, src, lambda: helpers.PortCC.gaussblur(src, sigma))
    if kind == "colour":
        return _colour_case(rng, seed)
    # a small 2-D mask on uchar / ushort
    w, h = _size(rng, 8), _size(rng, 8)
    dt = rng.choice([np.uint8, np.uint16])
    src = helpers.lcg_image(w, h, bands, dt, seed)
    mw, mh = rng.choice([1, 3, 5, 7, 9]), rng.choice([3, 5, 7]) if dt == np.uint8 else rng.choice([3, 5])
    if dt == np.uint16:
        mw = min(mw, 5)
    m = np.array([[rng.randrange(-3, 12) for _ in range(mw)] for _ in range(mh)], dtype=np.float64)
    scale = max(1, int(m.sum()))
    im = Image.new_from_array(src)

    def ref2():
        if helpers.have_ref():
            return helpers.Ref.run_mask("conv", src, m, scale, 0.0, "precision=integer")
        return helpers.PortCC.conv(src, m, scale=scale, precision="integer")
    return (kind, w, h, bands, dt.__name__, m.tolist(), scale), lambda: im.conv(m, scale=scale, precision="integer"), ref2


@pytest.mark.parametrize("kind,count,seed", [("reduce", 60, 501), ("shrink", 30, 502), ("blur", 40, 503),
                                             ("convsep", 30, 504), ("conv", 30, 505), ("resize", 14, 506),
                                             ("float", 40, 507), ("upsize", 24, 508), ("blur16", 24, 509),
                                             ("colour", 90, 510)])
def test_fuzz_dispatch(kind, count, seed):
    rng = random.Random(seed)
    lib = libvips_amd.lib
    kernels = {}
    for _ in range(count):
        desc, call, ref = _case(rng, kind)
        lib.vips_hip_gate_reset()
        lib.vips_hip_gate_enable(1)
        try:
            got = call().numpy()
            report = libvips_amd.gate_report()
        finally:
            lib.vips_hip_gate_enable(0)
            lib.vips_hip_gate_reset()
        assert report, desc
        for k in report:
            kernels[k] = kernels.get(k, 0) + 1
        want = ref()
        assert got.shape == want.shape and got.dtype == want.dtype, (desc, got.shape, want.shape)
        if kind == "colour":
            # the rule of tests/test_colour_routes_gpu.py: bytes equal, but that NaN on both sides counts as equal
            from tests import colour_domains

            bad = colour_domains.differing(got, want)
            assert len(bad) == 0, (desc, dict(report), len(bad), bad[:4].tolist())
            continue
        if got.dtype == np.float32:  # (bit for bit, NaN-safe: the float paths are the reference's operations in its order)
            got, want = got.view(np.int32), want.view(np.int32)
        bad = np.argwhere(got != want)
        assert len(bad) == 0, (desc, dict(report), len(bad), bad[:4].tolist())
    # the sweep must have reached the fast kernels AND their fall-backs
    assert len(kernels) >= {"upsize": 1, "blur16": 2}.get(kind, 3), kernels
    if kind == "colour":
        # four of the five families of colour_route() (the fifth, colour_lab_lds, needs another cube-root table)
        assert len([k for k in COLOUR_GATES if k in kernels]) >= 4, kernels
