"""GPU parity: masks on the device -- vips_relational / vips_relational_const, vips_boolean / vips_boolean_const,
vips_ifthenelse with and without blend, vips_bandjoin / vips_bandjoin_const, vips_extract_band, vips_bandmean and
vips_bandbool (libvips_amd/csrc/logic.hip, ops_logic.cpp).

Everything is np.array_equal on the bytes, with dtype, shape and interpretation, against the compiled reference:
one-image operations through Ref.run / Ref.run_interp, operations on several images through the reference's command
line on .v files.  The sweeps over element sizes, band counts, row lengths round the streaming kernels' groups and a
block of them, on windows of larger frames and under both kernels, compare one-image operations with the reference
directly and the others with numpy models that the whole-domain tests pin to the reference; every sweep case asserts by
the gate report which logic_ kernel ran and that exactly one launch was made (casts are counted apart).

Kept out of the inputs, because the reference's answer there is its compiler's, not its specification: NaN and values
outside int in float operands of boolean and bandbool, shift counts outside 0 .. 31, signed blend operands beyond
+-2^22.  NaN is in the relational and the plain ifthenelse inputs.  Runs on the CPU too, on host fibers
(tests/test_emul_logic.py)."""
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
from tests.test_arith_gpu import extremes_of, gen_in_frames, noise, same

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not helpers.have_ref(), reason="oracle/_ref not built")]

lib = _ffi.lib
INTERP = helpers.INTERP
VIPS = os.path.join(helpers.ROOT, "oracle", "_ref", "bin", "vips")
ALL_DTYPES = [np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32, np.float32, np.float64]
INT_DTYPES = ALL_DTYPES[:6]
SWEEP_DTYPES = {1: np.uint8, 2: np.int16, 4: np.float32, 8: np.float64}
RELATIONAL = ["equal", "noteq", "less", "lesseq", "more", "moreeq"]
BOOLEAN = ["and", "or", "eor", "lshift", "rshift"]
NP_RELATIONAL = {"equal": np.equal, "noteq": np.not_equal, "less": np.less, "lesseq": np.less_equal, "more": np.greater,
                 "moreeq": np.greater_equal}
name_of = lambda d: np.dtype(d).name  # noqa: E731


@pytest.fixture(scope="module", autouse=True)
def _init():
    libvips_amd.init(0)


class gated(object):
    """with gated() as g: ...; g.ran: {gate name: launches} of this feature's kernels that ran inside, g.casts: the
    launches of vips_hip_cast."""

    def __enter__(self):
        lib.vips_hip_gate_reset()
        lib.vips_hip_gate_enable(1)
        self.ran = self.casts = None
        return self

    def __exit__(self, *exc):
        try:
            if exc[0] is None:
                report = libvips_amd.gate_report()
                self.ran = {k: n for k, (n, _) in report.items() if k.startswith("logic_")}
                self.casts = sum(n for k, (n, _) in report.items() if k == "cast")
                # nothing but this feature's kernels and casts
                assert set(report) <= set(self.ran) | {"cast"}, report
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
            os.environ["VIPS_HIP_NO_LOGIC_STREAM"] = "1"

    def __exit__(self, *exc):
        os.environ.pop("VIPS_HIP_NO_LOGIC_STREAM", None)
        return False


def vec(v):
    return " ".join(repr(float(x)) for x in np.atleast_1d(v))


def carray(c):
    c = np.atleast_1d(np.asarray(c, np.float64))
    return c.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), len(c), c


def sweep_widths(pel, out_es):
    """Widths 1, 3, 5, 15, 16, 17, 31, 33 and one block's worth of the streaming kernel's groups - 1 / + 0 / + 1 pel."""
    block = lib.vips_hip_logic_step(0) * lib.vips_hip_logic_step(1) // out_es  # elements of the output a block makes
    per_pel = max(1, pel // out_es)
    return sorted({1, 3, 5, 15, 16, 17, 31, 33} | {max(1, block // per_pel + d) for d in (-1, 0, 1)})


def over_the_grid(out_es, bands, groups_per_lane=1):
    """A square side whose image has a few more units of output than a capped grid takes in one step, the last ragged."""
    units = lib.vips_hip_logic_step(2) * lib.vips_hip_logic_step(0) + 700
    elems = units * groups_per_lane * (lib.vips_hip_logic_step(1) // out_es) + 3
    return int(math.isqrt(elems // bands)) + 1


def ref_cli(tmp_path, op, images, *args):
    """-> (array, interpretation) of `vips <op> in0.v in1.v ... out.v <args>`; RuntimeError with its words."""
    paths = []
    for i, (array, interp) in enumerate(images):
        paths.append(str(tmp_path / ("in%d.v" % i)))
        helpers.write_v(paths[-1], array, interp)
    out = str(tmp_path / "out.v")
    ins = [" ".join(paths)] if op == "bandjoin" else paths
    r = subprocess.run([VIPS, op] + ins + [out] + list(args), env=helpers.ref_cli_env(), stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True)
    if r.returncode != 0:
        raise RuntimeError(r.stderr.strip() or "vips %s failed" % op)
    return helpers.read_v(out)


def check_images(tmp_path, op, images, args, call, what, kernel=None, casts=None):
    """The device's result and header against the reference's command line, or both an error with the reference's words.
    call(list of Images) -> Image."""
    dev = [Image.new_from_array(a, i) for a, i in images]
    try:
        want, want_interp = ref_cli(tmp_path, op, images, *args)
    except RuntimeError as e:
        words = str(e).strip().splitlines()[-1]
        with pytest.raises(VipsHipError) as info:
            call(dev)
        assert str(info.value).strip() == words, (what, words, str(info.value))
        return None
    with gated() as g:
        out = call(dev)
        got = out.numpy()
    same(got, want, (op, args, what))
    assert lib.vips_hip_image_get_interpretation(out._h) == want_interp, (op, what, "interpretation")
    # ONE launch, whatever had to be matched
    assert (g.ran == {kernel: 1}) if kernel else (sum(g.ran.values()) == 1), (op, what, g.ran)
    assert casts is None or g.casts == casts, (op, what, g.casts)
    return got


def check_one(nick, src, args, call, what, interp=0, kernel=None):
    """A one-image operation against Ref.run_interp; call(Image) -> Image."""
    want, want_interp = Ref.run_interp(nick, src, args, interpretation=interp)
    with gated() as g:
        out = call(Image.new_from_array(src, interp))
        got = out.numpy()
    same(got, want, (nick, args, what))
    assert interp == 0 or lib.vips_hip_image_get_interpretation(out._h) == want_interp, (nick, what, "interpretation")
    assert (g.ran == {kernel: 1}) if kernel else (sum(g.ran.values()) == 1), (nick, what, g.ran)
    assert g.casts == 0
    return got


def pairs_u8():
    x, y = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8))
    return np.ascontiguousarray(x[:, :, None]), np.ascontiguousarray(y[:, :, None])


# ---------------------------------------------------------------- numpy models (pinned to the reference below)

def model_relational(op, a, b):
    """numpy's comparisons (NaN as in C).  Pinned to the reference by test_relational_every_uchar_pair and
    test_relational_formats (every format, the extremes, NaN), which compare this model with the pixels they got."""
    with np.errstate(invalid="ignore"):
        return np.where(NP_RELATIONAL[op](a, b), 255, 0).astype(np.uint8)


def model_boolean(op, a, b):
    """Two images of one format: the operation on the values promoted to int (floats truncated), the store truncates.
    Pinned to the reference by test_boolean_every_uchar_pair and test_boolean_formats (every format, counts 0 .. 31)."""
    out = np.int32 if a.dtype.kind == "f" else a.dtype
    x, y = (np.trunc(v).astype(np.int64) if v.dtype.kind == "f" else v.astype(np.int64) for v in (a, b))
    if op == "and":
        r = x & y
    elif op == "or":
        r = x | y
    elif op == "eor":
        r = x ^ y
    elif op == "lshift":
        r = (x & 0xFFFFFFFF) << y
    else:
        r = x >> y
    return (r & 0xFFFFFFFF).astype(np.uint32).astype(out) if np.dtype(out).itemsize == 4 else r.astype(out)


def model_select(c, a, b):
    """Pinned to the reference by test_ifthenelse_every_condition_value[plain] (every format, both kinds of condition)."""
    cc = c if c.shape[2] == a.shape[2] else np.repeat(c, a.shape[2], axis=2)
    return np.where(cc != 0, a, b)


def model_blend(c, a, b):
    """Pinned to the reference by test_ifthenelse_every_condition_value[blend]: every condition value, every format; for
    int images only on operands within +-2^22 (beyond them the reference's sum overflows int, which is no contract),
    and the sweeps that use this model stay within that range too (int16 is their widest signed format)."""
    cc = (c if c.shape[2] == a.shape[2] else np.repeat(c, a.shape[2], axis=2)).astype(np.int64)
    if a.dtype.kind == "f":
        v = cc / 255.0
        return (v * a.astype(np.float64) + (1.0 - v) * b.astype(np.float64)).astype(a.dtype)
    t = cc * a.astype(np.int64) + (255 - cc) * b.astype(np.int64) + 128
    if a.dtype == np.uint32:
        return ((t & 0xFFFFFFFF) // 255).astype(np.uint32)
    q = np.abs(t) // 255 * np.sign(t)  # C's division truncates toward zero
    return q.astype(a.dtype)


# ---------------------------------------------------------------- relational: whole domains, constants

@pytest.mark.parametrize("kernel", ["stream", "general"])
@pytest.mark.parametrize("op", RELATIONAL)
def test_relational_every_uchar_pair(tmp_path, op, kernel):
    a, b = pairs_u8()
    with general_kernel(kernel == "general"):
        got = check_images(tmp_path, "relational", [(a, INTERP["b-w"]), (b, INTERP["b-w"])], [op],
                           lambda d: d[0].relational(d[1], op), "all pairs", kernel="logic_" + kernel, casts=0)
    same(got, model_relational(op, a, b), "the model")


@pytest.mark.parametrize("op", RELATIONAL)
@pytest.mark.parametrize("dtype", ALL_DTYPES[1:], ids=name_of)
def test_relational_formats(tmp_path, op, dtype):
    """The format's extremes and NaN against themselves in another order."""
    a = noise(33, 9, dtype, 3, 11, with_extremes=True)
    b = np.ascontiguousarray(a.reshape(-1)[::-1].reshape(a.shape))
    b.ravel()[::3] = a.ravel()[::3]
    if np.dtype(dtype).kind == "f":
        a.ravel()[20:23] = [np.nan, 1.0, np.nan]
        b.ravel()[20:23] = [np.nan, np.nan, 2.0]
    got = check_images(tmp_path, "relational", [(a, INTERP["srgb"]), (b, INTERP["srgb"])], [op],
                       lambda d: d[0].relational(d[1], op), name_of(dtype), kernel="logic_stream", casts=0)
    same(got, model_relational(op, a, b), "the model")


def ref_const(nick, key, op, src, c, interp=0):
    return Ref.run_interp(nick, src, "%s=%s,c=%s" % (key, op, vec(c)), interpretation=interp)


@pytest.mark.parametrize("op", RELATIONAL)
@pytest.mark.parametrize("dtype", ALL_DTYPES, ids=name_of)
def test_relational_const(op, dtype):
    """Integral constants (the int comparison on integer images), fractions (the double one), negatives against unsigned
    formats, per-band vectors, a one-band image against three constants."""
    src = noise(33, 5, dtype, 3, 21, with_extremes=True)
    src.ravel()[40:46] = [0, 1, 2, 3, 100, 127]
    if np.dtype(dtype).kind == "f":
        src.ravel()[50:54] = [np.nan, 2.5, -0.0, 0.5]
    for c in (0, 128, -1, -1.5, 2.5, 1e10, [1, 128, -3], [0.5, 2, 2], [2, 2, 2]):
        check_one("relational_const", src, "relational=%s,c=%s" % (op, vec(c)), lambda im: im.relational(c, op),
                  (name_of(dtype), c), interp=INTERP["srgb"], kernel="logic_stream")
    one = np.ascontiguousarray(src[:, :, :1])
    check_one("relational_const", one, "relational=%s,c=%s" % (op, vec([1, 128, -3])), lambda im: im.relational([1, 128, -3], op),
              (name_of(dtype), "one band against three"), interp=INTERP["b-w"], kernel="logic_general")


def test_relational_pinned_corners():
    """uint against a negative constant: int constants become unsigned, -1.5 takes the double comparison; NaN compares
    false except under noteq; float pels against an integral constant compare as doubles."""
    u = np.array([0, 1, 4000000000, 4294967295], np.uint32).reshape(1, 4, 1)
    assert Image.new_from_array(u).more(-1).numpy().ravel().tolist() == [0, 0, 0, 0]
    assert Image.new_from_array(u).more(-1.5).numpy().ravel().tolist() == [255, 255, 255, 255]
    assert Ref.run("relational_const", u, "relational=more,c=-1").ravel().tolist() == [0, 0, 0, 0]
    assert Ref.run("relational_const", u, "relational=more,c=-1.5").ravel().tolist() == [255, 255, 255, 255]
    f = np.array([1, np.nan, 2.5, -0.0], np.float32).reshape(1, 4, 1)
    want = {"equal": [0, 0, 0, 255], "noteq": [255, 255, 255, 0], "less": [0, 0, 0, 0], "moreeq": [255, 0, 255, 255]}
    for op, values in want.items():
        assert Image.new_from_array(f).relational(0, op).numpy().ravel().tolist() == values, op
        assert Ref.run("relational_const", f, "relational=%s,c=0" % op).ravel().tolist() == values, op
    g = np.array([16777216.0, 16777218.0], np.float32).reshape(1, 2, 1)
    assert Image.new_from_array(g).more(16777217).numpy().ravel().tolist() == [0, 255]


# ---------------------------------------------------------------- boolean

@pytest.mark.parametrize("kernel", ["stream", "general"])
@pytest.mark.parametrize("op", BOOLEAN)
def test_boolean_every_uchar_pair(tmp_path, op, kernel):
    a, b = pairs_u8()
    if op in ("lshift", "rshift"):
        b = b & 31  # counts 0 .. 31
    with general_kernel(kernel == "general"):
        got = check_images(tmp_path, "boolean", [(a, INTERP["b-w"]), (b, INTERP["b-w"])], [op],
                           lambda d: d[0].boolean(d[1], op), "all pairs", kernel="logic_" + kernel, casts=0)
    same(got, model_boolean(op, a, b), "the model")


def boolean_operands(dtype, seed, shift):
    """Noise with the extremes; floats inside int's range, fractions included; counts 0 .. width - 1 for the shifts."""
    a = noise(33, 9, dtype, 3, seed, with_extremes=True, finite=True)
    b = noise(33, 9, dtype, 3, seed + 2, with_extremes=True, finite=True)
    if np.dtype(dtype).kind == "f":
        a, b = (np.clip(v, -2e9, 2e9).astype(dtype) for v in (a, b))
    if shift:
        width = 32 if np.dtype(dtype).kind == "f" else min(32, 8 * np.dtype(dtype).itemsize if np.dtype(dtype).itemsize == 4 else 32)
        b = (np.arange(b.size).reshape(b.shape) % width).astype(dtype)
    return a, b


@pytest.mark.parametrize("op", BOOLEAN)
@pytest.mark.parametrize("dtype", ALL_DTYPES[1:], ids=name_of)
def test_boolean_formats(tmp_path, op, dtype):
    a, b = boolean_operands(dtype, 31, op in ("lshift", "rshift"))
    got = check_images(tmp_path, "boolean", [(a, INTERP["srgb"]), (b, INTERP["srgb"])], [op],
                       lambda d: d[0].boolean(d[1], op), name_of(dtype), kernel="logic_stream", casts=0)
    same(got, model_boolean(op, a, b), "the model")


@pytest.mark.parametrize("op", BOOLEAN)
@pytest.mark.parametrize("dtype", ALL_DTYPES, ids=name_of)
def test_boolean_const(op, dtype):
    a, _ = boolean_operands(dtype, 41, False)
    shift = op in ("lshift", "rshift")
    for c in ((1, 9, 31, [0, 7, 30], 1.5) if shift else (1, 1.5, 255, -1, 0x55AA55, [1, 0xF0, -256], [3, 3, 3])):
        check_one("boolean_const", a, "boolean=%s,c=%s" % (op, vec(c)), lambda im: im.boolean(c, op), (name_of(dtype), c),
                  interp=INTERP["srgb"], kernel="logic_stream")
    one = np.ascontiguousarray(a[:, :, :1])
    c = [1, 2, 3]
    check_one("boolean_const", one, "boolean=%s,c=%s" % (op, vec(c)), lambda im: im.boolean(c, op),
              (name_of(dtype), "one band against three"), interp=INTERP["b-w"], kernel="logic_general")


def test_boolean_pinned_corners(tmp_path):
    """char -128 >> 1 is -64 (arithmetic), uchar 8 << 9 is 0 (int, truncated at the store), & 1.5 is & 1."""
    c = np.array([-128, -1, 64, 127], np.int8).reshape(1, 4, 1)
    one = np.ones_like(c)
    assert Image.new_from_array(c).rshift(Image.new_from_array(one)).numpy().ravel().tolist() == [-64, -1, 32, 63]
    assert ref_cli(tmp_path, "boolean", [(c, 1), (one, 1)], "rshift")[0].ravel().tolist() == [-64, -1, 32, 63]
    assert Image.new_from_array(c).lshift(Image.new_from_array(one)).numpy().ravel().tolist() == [0, -2, -128, -2]
    assert ref_cli(tmp_path, "boolean", [(c, 1), (one, 1)], "lshift")[0].ravel().tolist() == [0, -2, -128, -2]
    assert (Image.new_from_array(c) >> 1).numpy().ravel().tolist() == [-64, -1, 32, 63]
    u = np.array([8, 1, 255], np.uint8).reshape(1, 3, 1)
    assert (Image.new_from_array(u) << 9).numpy().ravel().tolist() == [0, 0, 0]
    assert Ref.run("boolean_const", u, "boolean=lshift,c=9").ravel().tolist() == [0, 0, 0]
    assert (Image.new_from_array(u) & 1.5).numpy().ravel().tolist() == [0, 1, 1]
    assert Ref.run("boolean_const", u, "boolean=and,c=1.5").ravel().tolist() == [0, 1, 1]


# ---------------------------------------------------------------- two images: matching

PAIRS = [(np.uint8, np.int8), (np.uint8, np.uint16), (np.uint16, np.int16), (np.uint32, np.int32), (np.uint8, np.float32),
         (np.float32, np.float64)]


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: "%s-%s" % (name_of(p[0]), name_of(p[1])))
def test_binary_format_pairs(tmp_path, pair):
    """vips__formatalike, both orders: one cast (or two), one launch."""
    a, b = (noise(21, 9, t, 3, seed, with_extremes=True, finite=True) for t, seed in zip(pair, (51, 53)))
    if np.dtype(pair[1]).kind == "f":
        a, b = (np.clip(v, -2e9, 2e9).astype(v.dtype) for v in (a, b))
    for x, y in ((a, b), (b, a)):
        for op in ("less", "equal"):
            check_images(tmp_path, "relational", [(x, INTERP["srgb"]), (y, INTERP["srgb"])], [op],
                         lambda d: d[0].relational(d[1], op), (op, pair))
        for op in ("and", "eor"):
            check_images(tmp_path, "boolean", [(x, INTERP["srgb"]), (y, INTERP["srgb"])], [op],
                         lambda d: d[0].boolean(d[1], op), (op, pair))


def test_binary_bands_sizes_and_headers(tmp_path):
    """vips__bandalike: one band against three in both orders, three against four refused in the reference's words;
    vips__sizealike: 7 x 5 against 4 x 9; the header for mixed interpretations."""
    one, three = (noise(9, 7, np.uint8, 1, 61), INTERP["b-w"]), (noise(9, 7, np.uint8, 3, 63), INTERP["srgb"])
    four = (noise(9, 7, np.uint8, 4, 65), INTERP["srgb"])
    multi = (noise(9, 7, np.uint16, 3, 66), INTERP["multiband"])
    for nick, op, call in (("relational", "more", lambda d: d[0].more(d[1])), ("boolean", "or", lambda d: d[0].orimage(d[1]))):
        check_images(tmp_path, nick, [one, three], [op], call, "1 against 3", kernel="logic_general")
        check_images(tmp_path, nick, [three, one], [op], call, "3 against 1", kernel="logic_general")
        check_images(tmp_path, nick, [three, multi], [op], call, "srgb, multiband")
        check_images(tmp_path, nick, [multi, three], [op], call, "multiband, srgb")
        assert check_images(tmp_path, nick, [three, four], [op], call, "3 against 4") is None
        for dtype in (np.uint8, np.float32):
            a, b = (noise(7, 5, dtype, 3, 67), INTERP["srgb"]), (noise(4, 9, dtype, 3, 69), INTERP["srgb"])
            check_images(tmp_path, nick, [a, b], [op], call, "7x5 against 4x9", kernel="logic_general")
            check_images(tmp_path, nick, [b, a], [op], call, "4x9 against 7x5", kernel="logic_general")
        a, b = (noise(7, 5, np.int16, 1, 71), INTERP["b-w"]), (noise(4, 9, np.uint8, 3, 73), INTERP["srgb"])
        check_images(tmp_path, nick, [a, b], [op], call, "7x5x1 short against 4x9x3 uchar", casts=1)


# ---------------------------------------------------------------- ifthenelse

@pytest.mark.parametrize("blend", [False, True], ids=["plain", "blend"])
@pytest.mark.parametrize("dtype", ALL_DTYPES, ids=name_of)
def test_ifthenelse_every_condition_value(tmp_path, dtype, blend):
    """Every uchar condition value against the format's extremes (blend: signed operands within +-2^22, uint over its
    whole range), an n-band condition and a one-band condition over three bands."""
    dtype = np.dtype(dtype)
    a = noise(256, 4, dtype, 3, 81, with_extremes=True, finite=True)
    b = noise(256, 4, dtype, 3, 83, with_extremes=True, finite=True)
    if not blend and dtype.kind == "f":
        a.ravel()[9] = np.nan
    if blend and dtype.kind == "f":
        a, b = (np.clip(v, -1e30, 1e30).astype(dtype) for v in (a, b))
    if blend and dtype == np.int32:
        a, b = (np.clip(v, -(1 << 22), 1 << 22) for v in (a, b))
    cn = np.empty((4, 256, 3), np.uint8)
    for k in range(3):
        cn[:, :, k] = (np.arange(256) + 85 * k) & 255
    c1 = np.ascontiguousarray(cn[:, :, :1])
    model = model_blend if blend else model_select
    args = ["--blend"] if blend else []
    for c, what in ((cn, "n bands"), (c1, "one band")):
        got = check_images(tmp_path, "ifthenelse", [(c, INTERP["b-w"]), (a, INTERP["srgb"]), (b, INTERP["srgb"])], args,
                           lambda d: d[0].ifthenelse(d[1], d[2], blend=blend), (dtype.name, what), kernel="logic_select_stream", casts=0)
        same(got, model(c, a, b), "the model")


def test_ifthenelse_pinned_corners(tmp_path):
    """A float condition goes through the saturating cast; the two blend vectors."""
    cond = np.array([0.5, 0.999, 1.0, -3.0, 300.0], np.float32).reshape(1, 5, 1)
    then, else_ = np.full((1, 5, 1), 7, np.uint8), np.full((1, 5, 1), 9, np.uint8)
    want = [9, 9, 7, 9, 7]
    with gated() as g:
        got = Image.new_from_array(cond).ifthenelse(Image.new_from_array(then), Image.new_from_array(else_)).numpy()
    assert got.ravel().tolist() == want and sum(g.ran.values()) == 1 and g.casts == 1
    assert ref_cli(tmp_path, "ifthenelse", [(cond, 1), (then, 1), (else_, 1)])[0].ravel().tolist() == want
    v = np.array([0, 255, 100, 1], np.uint8).reshape(1, 4, 1)
    for dtype, a, b, want in ((np.int16, -7, 3, [3, -6, 0, 3]), (np.uint32, 4000000000, 3, [3, 8206866, 2227615, 15686278])):
        ia, ib = np.full((1, 4, 1), a, dtype), np.full((1, 4, 1), b, dtype)
        got = Image.new_from_array(v).ifthenelse(Image.new_from_array(ia), Image.new_from_array(ib), blend=True).numpy()
        assert got.ravel().tolist() == want, (dtype, got.ravel().tolist())
        assert ref_cli(tmp_path, "ifthenelse", [(v, 1), (ia, 1), (ib, 1)], "--blend")[0].ravel().tolist() == want


def test_ifthenelse_matching(tmp_path):
    """Bands and sizes over all three images, then / else to their common format, a 3-band condition with one-band
    operands, a one-band condition over five bands (the streaming kernel's run-time form), the header, constants as pyvips
    makes them."""
    c1, c3 = (noise(9, 7, np.uint8, 1, 91) & 1, INTERP["b-w"]), (noise(9, 7, np.uint8, 3, 93) & 1, INTERP["srgb"])
    a3, b3 = (noise(9, 7, np.uint8, 3, 95), INTERP["srgb"]), (noise(9, 7, np.int16, 3, 97), INTERP["multiband"])
    a1, b1 = (noise(9, 7, np.uint16, 1, 99), INTERP["b-w"]), (noise(9, 7, np.uint16, 1, 101), INTERP["b-w"])
    a5, b5 = (noise(9, 7, np.float32, 5, 103), INTERP["multiband"]), (noise(9, 7, np.float32, 5, 105), INTERP["multiband"])
    small = (noise(4, 9, np.uint8, 3, 107), INTERP["srgb"])
    four = (noise(9, 7, np.uint8, 4, 109), INTERP["srgb"])
    call = lambda d: d[0].ifthenelse(d[1], d[2])  # noqa: E731
    for blend in (False, True):
        args = ["--blend"] if blend else []
        call = lambda d: d[0].ifthenelse(d[1], d[2], blend=blend)  # noqa: E731
        check_images(tmp_path, "ifthenelse", [c1, a3, b3], args, call, "uchar and short", casts=1)
        check_images(tmp_path, "ifthenelse", [c3, a1, b1], args, call, "3-band condition, one-band operands", kernel="logic_select_general")
        check_images(tmp_path, "ifthenelse", [c3, a1, b3], args, call, "one-band then")
        check_images(tmp_path, "ifthenelse", [c1, a5, b5], args, call, "one band over five", kernel="logic_select_stream")
        check_images(tmp_path, "ifthenelse", [c1, a3, small], args, call, "sizes", kernel="logic_select_general")
        check_images(tmp_path, "ifthenelse", [small, a3, a3], args, call, "a small condition", kernel="logic_select_general")
        assert check_images(tmp_path, "ifthenelse", [c1, a3, four], args, call, "3 against 4") is None
    im, cond = Image.new_from_array(a3[0], "srgb"), Image.new_from_array(c1[0], "b-w")
    same(cond.ifthenelse(im, 0).numpy(), np.where(c1[0] != 0, a3[0], 0).astype(np.uint8), "a number")
    same(cond.ifthenelse([1, 2, 300], im).numpy(), np.where(c1[0] != 0, np.array([1, 2, 255], np.uint8), a3[0]), "a list")
    same(cond.ifthenelse(7, 9).numpy(), np.where(c1[0] != 0, 7, 9).astype(np.uint8), "two numbers")


# ---------------------------------------------------------------- the band operations

def test_bandjoin(tmp_path):
    """2, 3 and 8 images of mixed formats, bands and sizes in ONE launch; one image is a copy."""
    shapes = [(9, 7, 3, np.uint8, "srgb"), (9, 7, 1, np.uint8, "b-w"), (4, 9, 2, np.int16, "multiband"), (9, 7, 1, np.uint16, "b-w"),
              (5, 5, 4, np.uint8, "srgb"), (9, 7, 1, np.int8, "b-w"), (9, 7, 2, np.uint8, "multiband"), (1, 1, 1, np.uint8, "b-w")]
    images = [(noise(w, h, t, b, 200 + i, with_extremes=w > 1), INTERP[interp]) for i, (w, h, b, t, interp) in enumerate(shapes)]
    call = lambda d: d[0].bandjoin(d[1:])  # noqa: E731
    for kernel in ("stream", "general"):
        with general_kernel(kernel == "general"):
            check_images(tmp_path, "bandjoin", images[:2], [], call, "3 + 1 uchar", kernel="logic_band_" + ("pels" if kernel == "stream" else kernel), casts=0)
            check_images(tmp_path, "bandjoin", images[:3], [], call, "three, mixed")
            check_images(tmp_path, "bandjoin", images, [], call, "eight, mixed")
    for dtype in (np.uint16, np.float32, np.float64):
        pair = [(noise(17, 3, dtype, 2, 231), INTERP["multiband"]), (noise(17, 3, dtype, 3, 233), INTERP["srgb"])]
        check_images(tmp_path, "bandjoin", pair, [], call, name_of(dtype), kernel="logic_band_pels", casts=0)
    with gated() as g:
        got = Image.new_from_array(images[0][0], "srgb").bandjoin([]).numpy()
    same(got, images[0][0], "one image")
    assert g.ran == {}
    z = (noise(5, 4, np.float32, 1, 15) + 1j * noise(5, 4, np.float32, 1, 17)).astype(np.complex64)
    with pytest.raises(VipsHipError, match="image must be non-complex"):
        Image.new_from_array(z).bandjoin(Image.new_from_array(z))


@pytest.mark.parametrize("dtype", ALL_DTYPES, ids=name_of)
def test_bandjoin_const(dtype):
    src = noise(33, 5, dtype, 3, 241, with_extremes=True)
    for c in ([255], [1.5, -300], [0, 1, 2, 70000.7], [1, 2, 3, 4, 5]):
        # (three bands and up to four constants: whole pels from dwords; five constants: the gathering kernel)
        check_one("bandjoin_const", src, "c=%s" % vec(c), lambda im: im.bandjoin(c), (name_of(dtype), c), interp=INTERP["srgb"],
                  kernel="logic_band_pels" if len(c) <= 4 else "logic_band_stream")
    if np.dtype(dtype) == np.int8:
        got = Image.new_from_array(src).bandjoin([1.5, -300]).numpy()
        assert got[0, 0, 3:].tolist() == [1, -128]


@pytest.mark.parametrize("dtype", ALL_DTYPES, ids=name_of)
def test_extract_band_bandmean_bandbool(dtype):
    """Every band and run of bands of five; the means and folds of 1 .. 5 bands, extremes included (for float images
    within int's range for bandbool)."""
    dtype = np.dtype(dtype)
    for bands in (1, 2, 3, 4, 5):
        src = noise(33, 5, dtype, bands, 250 + bands, with_extremes=True, finite=True)
        src.ravel()[:bands] = extremes_of(dtype)[0]  # a pel of nothing but the first extreme: the mean must not wrap
        copy = bands == 1
        for nick, call in (("bandmean", lambda im: im.bandmean()),):
            want, want_interp = Ref.run_interp(nick, src, "", interpretation=INTERP["multiband"])
            with gated() as g:
                got = call(Image.new_from_array(src)).numpy()
            same(got, want, (nick, dtype.name, bands))
            assert g.ran == ({} if copy else {"logic_band_stream": 1}), g.ran
        quiet = np.clip(src, -2e9, 2e9).astype(dtype) if dtype.kind == "f" else src
        for op in ("and", "or", "eor"):
            want = Ref.run("bandbool", quiet, "boolean=" + op)
            with gated() as g:
                got = Image.new_from_array(quiet).bandbool(op).numpy()
            same(got, want, ("bandbool", op, dtype.name, bands))
            assert g.ran == ({} if copy else {"logic_band_stream": 1}), g.ran
        for band in range(bands):
            for n in range(1, bands - band + 1):
                want, want_interp = Ref.run_interp("extract_band", src, "band=%d,n=%d" % (band, n), interpretation=INTERP["srgb"])
                with gated() as g:
                    out = Image.new_from_array(src, "srgb").extract_band(band, n)
                    got = out.numpy()
                same(got, want, ("extract_band", dtype.name, bands, band, n))
                assert lib.vips_hip_image_get_interpretation(out._h) == want_interp
                # (from pels of 2 .. 4 bands: whole pels from dwords; of five: the gathering kernel)
                assert g.ran == ({} if n == bands else {"logic_band_pels" if bands <= 4 else "logic_band_stream": 1}), g.ran


def test_bandmean_pinned_corners():
    src = np.array([[-1, -2, -2], [-128, -128, -127], [127, 127, 126]], np.int8).reshape(1, 3, 3)
    assert Image.new_from_array(src).bandmean().numpy().ravel().tolist() == [-2, -128, 127]
    assert Ref.run("bandmean", src).ravel().tolist() == [-2, -128, 127]
    wide = np.array([[4294967295, 4294967295, 4294967294], [1, 2, 2]], np.uint32).reshape(1, 2, 3)
    same(Image.new_from_array(wide).bandmean().numpy(), Ref.run("bandmean", wide), "uint: a 64-bit sum")


# ---------------------------------------------------------------- both kernels over geometries, on windows of frames

def rows_on_dwords(w, h, pel, es, margin, pad):
    """Whether the rows of gen_in_frames' window start on dwords (its layout: `margin` elements, or max(4, es) bytes, before
    a row's first pel, strides rounded up to that unit; one row has no stride)."""
    m, unit = (max(4, es), max(4, es)) if margin % 4 == 0 else (margin * es, es)
    stride = (m + w * pel + pad + unit - 1) // unit * unit
    return (stride + m) % 4 == 0 and (h == 1 or stride % 4 == 0)


def gen_case(nick, src):
    """-> (args for Ref.run, generate call, output dtype, output bands) of a one-image operation on src."""
    bands = src.shape[2]
    itemsize = src.dtype.itemsize
    c = [100.0, 7.0, -3.5, 0.0, 1.0][:bands] if bands > 1 else [100.0]
    if nick == "relational_const":
        p, n, keep = carray(c)
        return "relational=more,c=" + vec(c), lambda i, o: (keep, lib.vips_hip_relational_const_gen(4, p, n, i, o))[1], np.uint8, bands
    if nick == "boolean_const":
        p, n, keep = carray(c)
        out = np.int32 if src.dtype.kind == "f" else src.dtype
        return "boolean=eor,c=" + vec(c), lambda i, o: (keep, lib.vips_hip_boolean_const_gen(2, p, n, i, o))[1], out, bands
    if nick == "bandjoin_const":
        p, n, keep = carray([9.0, 200.0])
        return "c=9 200", lambda i, o: (keep, lib.vips_hip_bandjoin_const_gen(p, n, i, o))[1], src.dtype, bands + 2
    if nick == "extract_band":
        band, n = (1, bands - 1) if bands > 1 else (0, 1)
        return "band=%d,n=%d" % (band, n), lambda i, o: lib.vips_hip_extract_band_gen(band, i, o), src.dtype, n
    if nick == "bandmean":
        return "", lib.vips_hip_bandmean_gen, src.dtype, 1
    assert nick == "bandbool" and itemsize
    out = np.int32 if src.dtype.kind == "f" else src.dtype
    return "boolean=eor", lambda i, o: lib.vips_hip_bandbool_gen(2, i, o), out, 1


GEN_KERNELS = {"relational_const": "logic_", "boolean_const": "logic_", "bandjoin_const": "logic_band_", "extract_band": "logic_band_",
               "bandmean": "logic_band_", "bandbool": "logic_band_"}


@pytest.mark.parametrize("kernel", ["stream", "general", "unaligned"])
@pytest.mark.parametrize("bands", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("es", [1, 2, 4, 8])
@pytest.mark.parametrize("nick", sorted(GEN_KERNELS))
def test_one_image_sweep(nick, es, bands, kernel):
    """stream: rows on dwords; general: the same under VIPS_HIP_NO_LOGIC_STREAM; unaligned: rows that start one element
    after a dword and odd strides, which the streams decline where that puts the output's rows (the band kernels) or
    either side's (the pointwise ones) off dwords.  The window's frame must stay untouched (gen_in_frames)."""
    dtype = np.dtype(SWEEP_DTYPES[es])
    if nick in ("extract_band", "bandmean", "bandbool") and bands == 1 and nick != "extract_band":
        bands = 6  # (one band is a copy made by the caller: six bands instead, past the templated counts)
    for w in sweep_widths(es * bands, es):
        for h in (1, 2, 3):
            src = noise(w, h, dtype, bands, 1000 + w)
            args, call, out_dtype, out_bands = gen_case(nick, src)
            margin = 1 if kernel == "unaligned" else 4
            with general_kernel(kernel == "general"), gated() as g:
                got = gen_in_frames(src, out_dtype, out_bands, call, margin)
            in_on = rows_on_dwords(w, h, es * bands, es, margin, 5)
            out_on = rows_on_dwords(w, h, np.dtype(out_dtype).itemsize * out_bands, np.dtype(out_dtype).itemsize, margin, 7)
            streams = kernel != "general" and out_on and (in_on or GEN_KERNELS[nick] == "logic_band_")
            assert kernel != "stream" or streams
            # bandjoin_const of 1 .. 4 bands (two constants) and extract_band from 2 .. 4 bands: whole pels from dwords
            pels = in_on and ((nick == "bandjoin_const" and bands <= 4) or (nick == "extract_band" and 2 <= bands <= 4))
            assert g.ran == {GEN_KERNELS[nick] + (("pels" if pels else "stream") if streams else "general"): 1}, (g.ran, nick, es, bands, w, h)
            same(got, Ref.run(nick, src, args), (nick, kernel, es, bands, w, h))


@pytest.mark.parametrize("kernel", ["stream", "general"])
@pytest.mark.parametrize("bands", [1, 3])
@pytest.mark.parametrize("es", [1, 2])
def test_one_row_sweep(es, bands, kernel):
    """One row is nothing away from a next one, so its stride has no say (the rule this family shares with arithmetic):
    more_const on a one-row window that starts on a dword, out of frames whose strides are no multiple of 4, and `and`
    of two one-row images, whose strides are their rows' bytes whatever those are, stream; the general kernel gives
    the same bytes."""
    dtype = np.dtype(SWEEP_DTYPES[es])
    name = "logic_stream" if kernel == "stream" else "logic_general"
    for w in sweep_widths(es * bands, es):
        src = noise(w, 1, dtype, bands, 4000 + w)
        args, call, out_dtype, out_bands = gen_case("relational_const", src)
        with general_kernel(kernel == "general"), gated() as g:
            got = gen_in_frames(src, out_dtype, out_bands, call, 4, odd_stride=True)
        assert g.ran == {name: 1}, (g.ran, es, bands, w)
        same(got, Ref.run("relational_const", src, args), ("more_const", kernel, es, bands, w))
        other = noise(w, 1, dtype, bands, 4001 + w)
        ia, ib = Image.new_from_array(src), Image.new_from_array(other)
        with general_kernel(kernel == "general"), gated() as g:
            got = ia.andimage(ib).numpy()
        assert g.ran == {name: 1} and g.casts == 0, (g.ran, es, bands, w)
        same(got, model_boolean("and", src, other), ("and", kernel, es, bands, w))


@pytest.mark.parametrize("kernel", ["stream", "general"])
@pytest.mark.parametrize("bands", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("es", [1, 2, 4, 8])
def test_several_images_sweep(es, bands, kernel):
    """Whole images (rows that follow one another are one row to the streams) against the models: relational, boolean,
    ifthenelse plain and blended under an n-band and a one-band condition, bandjoin."""
    dtype = np.dtype(SWEEP_DTYPES[es])
    stream = kernel == "stream"
    for w in sweep_widths(es * bands, es):
        for h in (1, 2, 3):
            a, b = noise(w, h, dtype, bands, 3000 + w, finite=True), noise(w, h, dtype, bands, 3001 + w, finite=True)
            if dtype.kind == "f":
                a, b = np.clip(a, -2e9, 2e9).astype(dtype), np.clip(b, -2e9, 2e9).astype(dtype)
            cn, c1 = noise(w, h, np.uint8, bands, 3002 + w) & 0x81, noise(w, h, np.uint8, 1, 3003 + w) & 0x81
            ia, ib, icn, ic1 = (Image.new_from_array(v) for v in (a, b, cn, c1))
            what = (kernel, es, bands, w, h)
            one_band_streams = stream  # (whatever the band count: five bands take the kernel's run-time form)
            cases = [("logic_", stream, lambda: ia.less(ib), model_relational("less", a, b)),
                     ("logic_", stream, lambda: ia.eorimage(ib), model_boolean("eor", a, b)),
                     ("logic_select_", stream, lambda: icn.ifthenelse(ia, ib), model_select(cn, a, b)),
                     ("logic_select_", one_band_streams, lambda: ic1.ifthenelse(ia, ib), model_select(c1, a, b)),
                     ("logic_select_", stream, lambda: icn.ifthenelse(ia, ib, blend=True), model_blend(cn, a, b)),
                     ("logic_select_", one_band_streams, lambda: ic1.ifthenelse(ia, ib, blend=True), model_blend(c1, a, b)),
                     ("logic_band_", stream, lambda: ia.bandjoin(ib), np.concatenate([a, b], axis=2))]
            for i, (gate, streams, fn, want) in enumerate(cases):
                with general_kernel(not stream), gated() as g:
                    got = fn().numpy()
                # (bandjoin of two images of 1 .. 4 bands: whole pels from dwords)
                name = "pels" if gate == "logic_band_" and bands <= 4 else "stream"
                assert g.ran == {gate + (name if streams else "general"): 1} and g.casts == 0, (g.ran, i, what)
                same(got, want, (i, what))


def test_grid_stride():
    """One case a family just large enough that a lane of a capped grid takes a second unit."""
    side = over_the_grid(1, 3)
    a, b = noise(side, side, np.uint8, 3, 411), noise(side, side, np.uint8, 3, 413)
    c1 = noise(side, side, np.uint8, 1, 415) & 0x81
    assert -(-side * side * 3 // 16) > lib.vips_hip_logic_step(2) * lib.vips_hip_logic_step(0)
    ia, ib, ic = Image.new_from_array(a), Image.new_from_array(b), Image.new_from_array(c1)
    c = [100, 7, 200]
    cases = [("logic_stream", lambda: ia.more(ib), model_relational("more", a, b)),
             ("logic_stream", lambda: ia.more(c), model_relational("more", a, np.array(c).reshape(1, 1, 3))),
             ("logic_band_stream", lambda: ia.bandmean(), Ref.run("bandmean", a)),
             ("logic_band_pels", lambda: ia.bandjoin(255), Ref.run("bandjoin_const", a, "c=255")),
             ("logic_band_pels", lambda: ia[1], Ref.run("extract_band", a, "band=1")),
             ("logic_band_stream", lambda: ia.bandjoin([1, 2, 3, 4, 5]), Ref.run("bandjoin_const", a, "c=1 2 3 4 5"))]
    for gate, fn, want in cases:
        with gated() as g:
            got = fn().numpy()
        assert g.ran == {gate: 1}, (gate, g.ran)
        same(got, want, gate)
    # the select kernel's units under a one-band condition are three groups: a larger image for its second step
    side = over_the_grid(1, 3, 3)
    a, b = noise(side, side, np.uint8, 3, 417), noise(side, side, np.uint8, 3, 419)
    c1 = noise(side, side, np.uint8, 1, 421) & 0x81
    assert side * side // 16 > lib.vips_hip_logic_step(2) * lib.vips_hip_logic_step(0)
    with gated() as g:
        got = Image.new_from_array(c1).ifthenelse(Image.new_from_array(a), Image.new_from_array(b)).numpy()
    assert g.ran == {"logic_select_stream": 1}, g.ran
    same(got, model_select(c1, a, b), "select")


@pytest.mark.parametrize("nick", ["relational_const", "bandmean", "extract_band"])
def test_second_turn_of_the_streams_in_frames(nick):
    """Rows that stay rows: a window of a larger frame whose rows together have more units than the capped grid has
    lanes, so that a lane's second unit is on another row and elsewhere in it (for the constants: at another phase of
    the band vector); every row ends in a ragged unit, and nothing outside the window is written (gen_in_frames).
    Units: 16 bytes of output for logic_stream (relational_const) and logic_band_stream (bandmean), 16 pels of uchar
    for logic_band_pels (extract_band).  (ifthenelse has no region form -- vips_hip_ifthenelse takes whole images, whose
    rows are always joined -- so logic_select_stream cannot be given rows that stay rows; test_grid_stride turns it on
    a whole image.)"""
    lanes = lib.vips_hip_logic_step(2) * lib.vips_hip_logic_step(0)
    group = lib.vips_hip_logic_step(1)
    width = (4096 + 5) // 3 if nick == "relational_const" else 4096 + 5  # 4101 output elements a row
    out_elems = width * 3 if nick == "relational_const" else width
    units = -(-out_elems // group)
    height = lanes // units + 9
    assert out_elems % group and height > 1 and units * height > lanes and lanes % units and lanes % units * group % 3
    src = noise(width, height, np.uint8, 3, 431)
    args, call, out_dtype, out_bands = gen_case(nick, src)
    with gated() as g:
        got = gen_in_frames(src, out_dtype, out_bands, call, 4)
    assert g.ran == {{"relational_const": "logic_stream", "bandmean": "logic_band_stream", "extract_band": "logic_band_pels"}[nick]: 1}, g.ran
    same(got, Ref.run(nick, src, args), nick)


@pytest.mark.parametrize("blocks", [1, 3])
@pytest.mark.parametrize("nick", ["relational_const", "bandmean", "ifthenelse"])
def test_second_turn_of_the_general_kernels(nick, blocks):
    """The one-element-a-lane kernels with more rows than grid.y, which is the cap for rows of one block and a third of
    it for rows of three (the last ragged)."""
    threads, cap = lib.vips_hip_logic_step(0), lib.vips_hip_logic_step(2)
    out_elems = (blocks - 1) * threads + 63
    width = out_elems if nick == "bandmean" else out_elems // 3
    out_elems = width if nick == "bandmean" else width * 3
    in_flight = -(-cap // blocks)
    rows = in_flight + (3 if blocks == 1 else 2)
    assert -(-out_elems // threads) == blocks and out_elems % threads and rows > in_flight and (blocks == 1) == (in_flight == cap)
    src = noise(width, rows, np.int16, 3, 441)
    if nick == "ifthenelse":
        other, cond = noise(width, rows, np.int16, 3, 443), noise(width, rows, np.uint8, 1, 445) & 0x81
        with general_kernel(), gated() as g:
            got = Image.new_from_array(cond).ifthenelse(Image.new_from_array(src), Image.new_from_array(other)).numpy()
        assert g.ran == {"logic_select_general": 1}, g.ran
        same(got, model_select(cond, src, other), (nick, blocks))
        return
    args, call, out_dtype, out_bands = gen_case(nick, src)
    with general_kernel(), gated() as g:
        got = gen_in_frames(src, out_dtype, out_bands, call, 4)
    assert g.ran == {GEN_KERNELS[nick] + "general": 1}, g.ran
    same(got, Ref.run(nick, src, args), (nick, blocks))


# ---------------------------------------------------------------- errors, operators, refusals

def test_errors_are_the_references(tmp_path):
    src = noise(9, 7, np.uint8, 3, 13)
    im = Image.new_from_array(src, "srgb")
    for nick, args, fn in (("extract_band", "band=3", lambda: im.extract_band(3)), ("extract_band", "band=1,n=3", lambda: im.extract_band(1, 3)),
                           ("bandbool", "boolean=lshift", lambda: im.bandbool("lshift")),
                           ("bandbool", "boolean=rshift", lambda: im.bandbool("rshift")),
                           ("relational_const", "relational=more,c=1 2", lambda: im.more([1, 2])),
                           ("boolean_const", "boolean=and,c=1 2 3 4", lambda: im & [1, 2, 3, 4])):
        with pytest.raises(RuntimeError) as ref:
            Ref.run(nick, src, args)
        with pytest.raises(VipsHipError) as dev:
            fn()
        # (Ref.run puts the operation's name before the reference's own message)
        assert nick + ": " + str(dev.value).strip() == str(ref.value).strip().splitlines()[-1], (str(ref.value), str(dev.value))
    z = (noise(5, 4, np.float32, 1, 15) + 1j * noise(5, 4, np.float32, 1, 17)).astype(np.complex64)
    for nick, args, fn in (("boolean_const", "boolean=and,c=1", lambda i: i & 1), ("bandbool", "boolean=and", lambda i: i.bandand())):
        with pytest.raises(RuntimeError) as ref:
            Ref.run(nick, z, args)
        with pytest.raises(VipsHipError) as dev:
            fn(Image.new_from_array(z))
        assert nick + ": " + str(dev.value).strip() == str(ref.value).strip().splitlines()[-1], (str(ref.value), str(dev.value))
    for fn in (lambda i: i.more(1), lambda i: i.more(i), lambda i: i.andimage(i), lambda i: i.ifthenelse(i, i), lambda i: i.bandmean(),
               lambda i: i.extract_band(0), lambda i: i.bandjoin(1)):
        with pytest.raises(VipsHipError, match="image must be non-complex"):
            fn(Image.new_from_array(z))


def test_operators():
    a, b = noise(9, 7, np.uint8, 3, 19), noise(9, 7, np.uint8, 3, 23)
    ia, ib = Image.new_from_array(a, "srgb"), Image.new_from_array(b, "srgb")
    for got, want in ((ia > ib, ia.more(ib)), (ia >= ib, ia.moreeq(ib)), (ia < ib, ia.less(ib)), (ia <= ib, ia.lesseq(ib)),
                      (ia > 128, ia.more(128)), (ia >= [1, 2, 3], ia.moreeq([1, 2, 3])), (ia < 7.5, ia.less(7.5)), (ia <= 0, ia.lesseq(0)),
                      (ia & ib, ia.andimage(ib)), (ia | ib, ia.orimage(ib)), (ia ^ ib, ia.eorimage(ib)), (ia & 15, ia.andimage(15)),
                      (15 & ia, ia.andimage(15)), (ia | [1, 2, 4], ia.orimage([1, 2, 4])), (ia ^ 255, ia.eorimage(255)),
                      (ia << 2, ia.lshift(2)), (ia >> 2, ia.rshift(2)), (ia >> (ib & 7), ia.rshift(ib & 7)),
                      (ia[1], ia.extract_band(1)), (ia[-1], ia.extract_band(2)), (ia[0:2], ia.extract_band(0, 2)), (ia[1:], ia.extract_band(1, 2))):
        same(got.numpy(), want.numpy(), "operator")
    same((~ia).numpy(), ~a, "~")
    same((ia > ib).ifthenelse(ia, ib).numpy(), np.maximum(a, b), "(a > b).ifthenelse(a, b)")
    same(ia.equal(ib).numpy(), model_relational("equal", a, b), "equal")
    same(ia.noteq(7).numpy(), model_relational("noteq", a, 7), "noteq")
    same(ia.bandand().numpy(), a[:, :, :1] & a[:, :, 1:2] & a[:, :, 2:], "bandand")
    same(ia.bandor().numpy(), a[:, :, :1] | a[:, :, 1:2] | a[:, :, 2:], "bandor")
    same(ia.bandeor().numpy(), a[:, :, :1] ^ a[:, :, 1:2] ^ a[:, :, 2:], "bandeor")
    with pytest.raises(IndexError):
        ia[3]
    # == and != on images are still identity, and an Image is hashable
    other = Image.new_from_array(a, "srgb")
    assert (ia == ia) is True and (ia == other) is False and (ia != other) is True and len({ia, other}) == 2


# ---------------------------------------------------------------- the libvips module's classes

needs_module = pytest.mark.skipif(not helpers.have_module(), reason="host/_build missing")


@needs_module
@pytest.mark.parametrize("strips", [False, True], ids=["whole", "strips"])
def test_module_logic_classes(strips):
    """relational_const_hip, boolean_const_hip, bandjoin_const_hip, extract_band_hip, bandmean_hip and bandbool_hip make
    the built-in operations' pixels and headers, whole and strip by strip (a small $VIPS_HIP_BUDGET, as
    tests/test_module.py)."""
    Ref.load_module()
    module = ctypes.CDLL(helpers.MODULE_LIB)
    height = 700 if strips else 50
    rgba = noise(400, height, np.uint8, 4, 301)
    grey = noise(400, height, np.uint16, 1, 303)
    signed = noise(400, height, np.int16, 3, 305, with_extremes=True)
    real = noise(400, height, np.float32, 3, 307)
    cases = [("relational_const", rgba, "relational=more,c=128"), ("relational_const", rgba, "relational=lesseq,c=1 128.5 -3 255"),
             ("relational_const", grey, "relational=noteq,c=1 2 3"), ("relational_const", real, "relational=less,c=0"),
             ("boolean_const", rgba, "boolean=and,c=15"), ("boolean_const", signed, "boolean=rshift,c=1 2 3"),
             ("boolean_const", real, "boolean=eor,c=255"), ("bandjoin_const", rgba, "c=255"), ("bandjoin_const", signed, "c=1.5 -300"),
             ("bandjoin_const", grey, "c=1 2 3 4 5"), ("extract_band", rgba, "band=1"), ("extract_band", rgba, "band=1,n=3"),
             ("extract_band", signed, "band=2"), ("bandmean", rgba, ""), ("bandmean", signed, ""), ("bandmean", real, ""),
             ("bandbool", rgba, "boolean=and"), ("bandbool", signed, "boolean=eor"), ("bandbool", real, "boolean=or")]
    if strips:
        os.environ["VIPS_HIP_BUDGET"] = "300k"
    before = module.vips_hip_module_strips_done()
    try:
        for nick, src, args in cases:
            got = Ref.run_interp(nick + "_hip", src, args, interpretation=INTERP["srgb"])
            want = Ref.run_interp(nick, src, args, interpretation=INTERP["srgb"])
            same(got[0], want[0], "%s_hip %s" % (nick, args))
            assert got[1] == want[1], (nick, args, "interpretation")
    finally:
        if strips:
            del os.environ["VIPS_HIP_BUDGET"]
    if strips:
        assert module.vips_hip_module_strips_done() - before >= 2 * len(cases), "not strip-mined"


@needs_module
def test_module_logic_errors_are_the_originals():
    Ref.load_module()
    src = noise(40, 30, np.uint8, 3, 309)
    z = (noise(5, 4, np.float32, 1, 15) + 1j * noise(5, 4, np.float32, 1, 17)).astype(np.complex64)
    for nick, image, args in (("relational_const", src, "relational=more,c=1 2"), ("boolean_const", src, "boolean=and,c=1 2 3 4"),
                              ("extract_band", src, "band=3"), ("extract_band", src, "band=1,n=3"), ("bandbool", src, "boolean=lshift"),
                              ("boolean_const", z, "boolean=and,c=1"), ("bandbool", z, "boolean=and")):
        with pytest.raises(RuntimeError) as ref:
            Ref.run(nick, image, args)
        with pytest.raises(RuntimeError) as hip:
            Ref.run(nick + "_hip", image, args)
        words = str(ref.value).strip().splitlines()[-1].split(": ", 2)[-1]
        assert words in str(hip.value), (str(ref.value), str(hip.value))
    # what the originals can do and the device path cannot is the originals': complex images, 33 constants
    same(Ref.run("relational_const_hip", z, "relational=equal,c=1"), Ref.run("relational_const", z, "relational=equal,c=1"), "complex")
    same(Ref.run("bandmean_hip", np.repeat(z, 2, axis=2), ""), Ref.run("bandmean", np.repeat(z, 2, axis=2), ""), "complex bandmean")
    one = noise(9, 7, np.uint8, 1, 311)
    many = " ".join(str(i) for i in range(33))
    same(Ref.run("relational_const_hip", one, "relational=more,c=" + many), Ref.run("relational_const", one, "relational=more,c=" + many), "33 constants")
