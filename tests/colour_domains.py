"""Inputs for the colour route tests (tests/test_colour_routes_gpu.py on the device and on host fibers,
tests/test_oracle_conv_colour.py for the port): whole domains where a space has one, lattices, stratified floats and
special values where it has not.  Everything is made from fixed seeds with numpy alone; every image has three bands
and a width that is a multiple of 4, so a whole image takes the 4-pixels-per-lane kernels.  Test infrastructure only."""
import functools

import numpy as np

# NaN, the infinities, both zeros, denormals, huge values, the values either side of an int32 index overflow (2^31
# itself, and 2^31 over the scale factors of the table lookups: 100000 for the cube-root table, 255 / 65535 / 32767
# for the encoders), the ends of the encoders' ranges
SPECIALS = np.array([
    np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-40, -1e-40, 1.4e-45, 1.17549435e-38, 1e30, -1e30, 3.4028235e38,
    2147483520.0, 2147483648.0, 2147483904.0, -2147483648.0, -2147483904.0, 4294967296.0,
    21474.834, 21474.838, 8421504.0, 8421505.0, 32768.25, 32768.75, 65538.0,
    1.0, -1.0, 0.5, 100.0, 255.0, 0.0031308, 50.0], dtype=np.float32)


def _bits(u):
    return np.ascontiguousarray(u, dtype=np.uint32).view(np.float32)


def special_grid(values=SPECIALS):
    """Every triple of `values`: (n, n * n, 3) float32 (n = 32: 32 x 1024 pixels)."""
    n = len(values)
    a, b, c = np.meshgrid(values, values, values, indexing="ij")
    return np.ascontiguousarray(np.stack([a, b, c], axis=-1).reshape(n, n * n, 3))


@functools.lru_cache(maxsize=None)
def cube():
    """Every uchar colour once: 4096 x 4096 x 3."""
    v = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([(v >> 16) & 255, (v >> 8) & 255, v & 255], axis=-1).astype(np.uint8).reshape(4096, 4096, 3)


def float_clip():
    """Float sRGB values round the clip to uchar the fast kernels start with: k + {0.49, 0.5, 0.999}, k - 0.5, the
    ends of the range, non-finite values.  Every channel swept over all of them with the others held, every triple of
    the range ends, seeded triples of everything: 1024 x 2072 pixels."""
    k = np.arange(256, dtype=np.float64)
    edges = np.array([255.5, 256.0, -0.5, -0.0, 1e30, np.nan, np.inf, -np.inf, -1e30, 300.0, -1.0, 0.0, 254.5, 255.0,
                      255.49, 255.999, 0.49, 0.5, 0.999, 127.5], dtype=np.float64)
    values = np.concatenate([k + 0.49, k + 0.5, k + 0.999, k - 0.5, edges]).astype(np.float32)
    held = np.array([0.0, 17.5, 128.49, 254.999, 255.5], dtype=np.float32)
    parts = []
    for c in range(3):
        for h1 in held:
            for h2 in held:
                p = np.empty((len(values), 3), np.float32)
                p[:, c] = values
                p[:, (c + 1) % 3] = h1
                p[:, (c + 2) % 3] = h2
                parts.append(p)
    parts.append(special_grid(edges.astype(np.float32)).reshape(-1, 3))
    rng = np.random.default_rng(611)
    have = sum(len(p) for p in parts)
    total = 1024 * 2072
    parts.append(values[rng.integers(0, len(values), size=(total - have, 3))])
    return np.ascontiguousarray(np.concatenate(parts).reshape(2072, 1024, 3))


def _ab_values(n, offset):
    """n short values: the ends, 0, +-1, and an even lattice between, moved by `offset`."""
    fixed = [-32768, -32767, -1, 0, 1, 32767]
    lattice = np.linspace(-32000, 32000, n - len(fixed)).astype(np.int64) + offset
    return np.concatenate([np.array(fixed, np.int64), lattice]).astype(np.int16)


def _labs_image(L, a_values, b_values):
    a, b = np.meshgrid(a_values, b_values, indexing="ij")
    pairs = np.stack([a.reshape(-1), b.reshape(-1)], axis=-1)
    out = np.empty((len(L), len(pairs), 3), np.int16)
    out[:, :, 0] = np.asarray(L, np.int16)[:, None]
    out[:, :, 1:] = pairs[None, :, :]
    return out


def labs_lattice(which):
    """LabS: 0: every L in 0 .. 32767 down the rows x 512 (a, b) pairs across (32 x 16 values with the ends, 0 and
    +-1 among them); 1: the same with the lattice moved by a prime and the axes' counts exchanged; 2: negative L
    (every 8th, and -32768 .. -1 all stand for L < 0) and every L of the dark arm (L < 8 * 327.67) and a little
    beyond x 2048 pairs."""
    if which == 0:
        return _labs_image(np.arange(32768), _ab_values(32, 0), _ab_values(16, 0))
    if which == 1:
        return _labs_image(np.arange(32768), _ab_values(16, 101), _ab_values(32, 211))
    L = np.concatenate([np.arange(-32768, 0, 8), np.arange(0, 2720)])
    return _labs_image(L, _ab_values(64, 37), _ab_values(32, 53))


def lab_float():
    """Lab float: L in [-20, 120], a and b in [-200, 200], seeded, 4064 rows of 4096; then every triple of SPECIALS
    (8 rows of 4096)."""
    rng = np.random.default_rng(612)
    n = 4064 * 4096
    out = np.empty((n, 3), np.float32)
    out[:, 0] = rng.uniform(-20.0, 120.0, n)
    out[:, 1] = rng.uniform(-200.0, 200.0, n)
    out[:, 2] = rng.uniform(-200.0, 200.0, n)
    return np.ascontiguousarray(np.concatenate([out, special_grid().reshape(-1, 3)]).reshape(4072, 4096, 3))


def _stratified(rng, count):
    """count x (every exponent x both signs x (mantissas 0, 1, 0x7fffff and seeded ones)): float32 bit patterns."""
    exps = np.arange(256, dtype=np.uint32)
    signs = np.array([0, 1], np.uint32)
    mant = rng.integers(0, 1 << 23, size=(256, 2, count), dtype=np.uint32)
    mant[:, :, 0] = 0
    mant[:, :, 1] = 1
    mant[:, :, 2] = 0x7FFFFF
    return ((signs[None, :, None] << 31) | (exps[:, None, None] << 23) | mant).reshape(-1)


def float_wide(space):
    """XYZ / scRGB float: per channel, every float exponent (0 and 255 too: denormals, infinities, NaNs) x both signs
    x 2048 mantissas (0, 1, 0x7fffff, seeded) with the other channels at ordinary values of the space; the same on
    all three channels at once; seeded raw bit patterns; ordinary values; every triple of SPECIALS.  2056 x 4096."""
    rng = np.random.default_rng({"xyz": 613, "scrgb": 614}[space])
    top = {"xyz": 110.0, "scrgb": 1.1}[space]
    parts = []
    for c in range(3):
        sweep = _stratified(rng, 2048)
        p = rng.uniform(-0.05 * top, top, size=(len(sweep), 3)).astype(np.float32)
        p[:, c] = _bits(sweep)
        parts.append(p)
    together = np.stack([_bits(rng.permutation(_stratified(rng, 2048))) for _ in range(3)], axis=-1)
    parts.append(together)
    parts.append(_bits(rng.integers(0, 1 << 32, size=(2 << 20, 3), dtype=np.uint64).astype(np.uint32)))
    parts.append(rng.uniform(-0.05 * top, top, size=(2 << 20, 3)).astype(np.float32))
    parts.append(special_grid().reshape(-1, 3))
    out = np.concatenate(parts)
    assert len(out) == 2056 * 4096, len(out)
    return np.ascontiguousarray(out.reshape(2056, 4096, 3))


def rgb16_wide():
    """RGB16 ushort: the grey diagonal over all 65536 values; each channel swept over all 65536 with the others at
    every pair of 0 / 0x8000 / 0xffff; a seeded block.  3840 x 1024."""
    v = np.arange(65536, dtype=np.uint16)
    parts = [np.stack([v, v, v], axis=-1)]
    for c in range(3):
        for h1 in (0, 0x8000, 0xFFFF):
            for h2 in (0, 0x8000, 0xFFFF):
                p = np.empty((65536, 3), np.uint16)
                p[:, c] = v
                p[:, (c + 1) % 3] = h1
                p[:, (c + 2) % 3] = h2
                parts.append(p)
    rng = np.random.default_rng(615)
    have = sum(len(p) for p in parts)
    parts.append(rng.integers(0, 65536, size=(3840 * 1024 - have, 3), dtype=np.uint16))
    return np.ascontiguousarray(np.concatenate(parts).reshape(3840, 1024, 3))


# source name -> (space the image is tagged with, maker, targets)
WIDE = {
    "labs0": ("labs", lambda: labs_lattice(0), ("srgb", "lab", "xyz", "scrgb", "rgb16", "b-w")),
    "labs1": ("labs", lambda: labs_lattice(1), ("srgb", "lab", "xyz", "scrgb", "rgb16", "b-w")),
    "labs-dark": ("labs", lambda: labs_lattice(2), ("srgb", "lab", "xyz", "scrgb", "rgb16", "b-w")),
    "lab": ("lab", lab_float, ("srgb", "xyz", "labs", "scrgb")),
    "xyz": ("xyz", lambda: float_wide("xyz"), ("lab", "labs", "srgb", "scrgb", "b-w", "grey16", "rgb16")),
    "scrgb": ("scrgb", lambda: float_wide("scrgb"), ("lab", "labs", "srgb", "xyz", "b-w", "grey16", "rgb16")),
    "rgb16": ("rgb16", rgb16_wide, ("lab", "labs", "xyz", "scrgb", "srgb", "b-w", "grey16")),
}
WIDE_CASES = [(name, target) for name in WIDE for target in WIDE[name][2]]


@functools.lru_cache(maxsize=1)
def wide_source(name):
    """(the image, its space); the last one made is kept, so cases run source by source make each once."""
    space, make, _ = WIDE[name]
    return make(), space


def layout_input(space, fmt, width, height, bands, seed):
    """A seeded image of `space` in format `fmt` with `bands` bands (the bands behind the third are extra bands)."""
    rng = np.random.default_rng(seed)
    shape = (height, width, bands)
    if space == "srgb" and fmt == "u8":
        return rng.integers(0, 256, size=shape, dtype=np.uint8)
    if space == "srgb":  # float sRGB: the byte range and a little more, with fractions
        return rng.uniform(-3.0, 259.0, size=shape).astype(np.float32)
    if space == "labs":
        s = rng.integers(-32768, 32768, size=shape, dtype=np.int16)
        s[:, :, 0] = np.abs(s[:, :, 0].astype(np.int32)).clip(0, 32767).astype(np.int16)
        return s
    if space == "lab":
        f = rng.uniform(-130.0, 130.0, size=shape).astype(np.float32)
        f[:, :, 0] = rng.uniform(-5.0, 105.0, size=shape[:2]).astype(np.float32)
        return f
    if space == "xyz":
        return rng.uniform(-5.0, 110.0, size=shape).astype(np.float32)
    if space == "scrgb":
        return rng.uniform(-0.1, 1.2, size=shape).astype(np.float32)
    if space == "rgb16":
        return rng.integers(0, 65536, size=shape, dtype=np.uint16)
    raise ValueError(space)


def differing(got, want):
    """The comparison rule of the colour route tests: same shape and dtype, bytes equal (signed zeros too), but that
    elements that are NaN on both sides count as equal -- sign and payload of an invalid-operation NaN are the
    machine's.  -> flat indices of the elements that differ."""
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, got.dtype, want.shape, want.dtype)
    g = np.ascontiguousarray(got).reshape(-1)
    w = np.ascontiguousarray(want).reshape(-1)
    if g.dtype.kind == "f":
        ne = g.view("u%d" % g.dtype.itemsize) != w.view("u%d" % w.dtype.itemsize)
        if ne.any():
            ne &= ~(np.isnan(g) & np.isnan(w))
    else:
        ne = g != w
    return np.flatnonzero(ne) if ne.any() else np.empty(0, np.int64)


def assert_same(got, want, what, src=None):
    bad = differing(got, want)
    if len(bad):
        bands = got.shape[2]
        lines = []
        for i in bad[:6]:
            y, x, b = np.unravel_index(i, got.shape)
            lines.append("(%d, %d) band %d: got %r, want %r%s" % (
                y, x, b, got[y, x].tolist(), want[y, x].tolist(),
                "" if src is None or src.shape[:2] != got.shape[:2] else ", from %r" % (src[y, x].tolist(),)))
        pixels = len(np.unique(bad // bands))
        raise AssertionError("%s: %d elements of %d pixels differ\n%s" % (what, len(bad), pixels, "\n".join(lines)))
