"""GPU parity: vips_recomb on the device (libvips_amd/csrc/recomb.hip, ops_recomb.cpp).

Every comparison is equality of dtype, shape, interpretation and bits against the compiled reference's command line
(`vips recomb in.v out.v m.v`, the matrix a .v file) -- float and double results as their integer views, so that -0.0
is not +0.0; positions where both sides are NaN count as equal.  Nothing has a tolerance: the kernels add the products
in the reference's order, in double, multiplies and adds separate.  Every case asserts by the gate report which of
the two kernels ran (recomb_stream, recomb_general) and that it was launched once.
Runs on the CPU too, on host fibers (tests/test_emul_arith2.py)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import libvips_amd
from libvips_amd import Image, VipsHipError, _ffi
from tests import helpers
from tests.test_arith2_gpu import same_bits
from tests.test_arith_gpu import ALL_DTYPES, gen_in_frames, noise

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not helpers.have_ref(), reason="oracle/_ref not built")]

lib = _ffi.lib
INTERP = helpers.INTERP
VIPS = os.path.join(helpers.ROOT, "oracle", "_ref", "bin", "vips")
STREAM_SHAPES = [(3, 3), (3, 1), (1, 3), (4, 4), (4, 3), (3, 4)]  # (mwidth, mheight)
STREAM_DTYPES = [np.uint8, np.uint16, np.float32]
SEPIA = [[0.393, 0.769, 0.189], [0.349, 0.686, 0.168], [0.272, 0.534, 0.131]]


def name_of(dtype):
    return np.dtype(dtype).name


@pytest.fixture(scope="module", autouse=True)
def _init():
    libvips_amd.init(0)


class gated(object):
    """with gated() as g: ...; g.ran: {gate name: launches} of the recomb kernels that ran inside."""

    def __enter__(self):
        lib.vips_hip_gate_reset()
        lib.vips_hip_gate_enable(1)
        self.ran = None
        return self

    def __exit__(self, *exc):
        try:
            if exc[0] is None:
                self.ran = {k: n for k, (n, _) in libvips_amd.gate_report().items() if k.startswith("recomb_")}
        finally:
            lib.vips_hip_gate_enable(0)
            lib.vips_hip_gate_reset()
        return False


class general_kernel(object):
    def __init__(self, on=True):
        self.on = on

    def __enter__(self):
        if self.on:
            os.environ["VIPS_HIP_NO_RECOMB_STREAM"] = "1"

    def __exit__(self, *exc):
        os.environ.pop("VIPS_HIP_NO_RECOMB_STREAM", None)
        return False


def matrix_of(mw, mh, seed):
    """Coefficients that are no floats, of both signs."""
    return np.random.default_rng(seed).normal(0.0, 1.5, (mh, mw))


def ref_recomb(tmp_path, src, m, interp=INTERP["multiband"]):
    """-> (array, interpretation); RuntimeError with the reference's words.  m: a 2D array of any real dtype."""
    paths = [str(tmp_path / n) for n in ("in.v", "m.v", "out.v")]
    helpers.write_v(paths[0], src, interp)
    m = np.asarray(m)
    helpers.write_v(paths[1], m[:, :, None] if m.ndim == 2 else m, INTERP["multiband"])
    r = subprocess.run([VIPS, "recomb", paths[0], paths[2], paths[1]], env=helpers.ref_cli_env(), stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True)
    if r.returncode != 0:
        raise RuntimeError(r.stderr.strip() or "vips recomb failed")
    return helpers.read_v(paths[2])


def check(tmp_path, src, m, kernel, what, interp=INTERP["multiband"], force_general=False, as_image=False):
    want, want_interp = ref_recomb(tmp_path, src, m, interp)
    arg = Image.new_from_array(np.asarray(m)[:, :, None]) if as_image else m
    with general_kernel(force_general), gated() as g:
        out = Image.new_from_array(src, interp).recomb(arg)
        got = out.numpy()
    same_bits(got, want, what)
    assert lib.vips_hip_image_get_interpretation(out._h) == want_interp, what
    assert g.ran == {"recomb_" + kernel: 1}, (what, g.ran)
    return got


def step_sizes():
    """(width, height): 1 x 1, 17 x 5, and one block's worth of the longest runs plus one pel, two plus one."""
    step = lib.vips_hip_recomb_step(0) * lib.vips_hip_recomb_step(2)
    assert step == 1024
    return [(1, 1), (17, 5), (41, 25), (683, 3)]  # 41 * 25 = step + 1, 683 * 3 = 2 * step + 1


# ---------------------------------------------------------------- the stream kernel

@pytest.mark.parametrize("dtype", STREAM_DTYPES, ids=name_of)
@pytest.mark.parametrize("shape", STREAM_SHAPES, ids=lambda s: "%dto%d" % s)
def test_stream_shapes(tmp_path, shape, dtype):
    mw, mh = shape
    m = matrix_of(mw, mh, 7 * mw + mh)
    for w, h in step_sizes():
        src = noise(w, h, dtype, mw, 100 + w, with_extremes=w * h * mw > 16, finite=True)
        check(tmp_path, src, m, "stream", (shape, name_of(dtype), w, h), interp=INTERP["srgb"] if mw == 3 else INTERP["multiband"])


@pytest.mark.parametrize("dtype", STREAM_DTYPES, ids=name_of)
def test_forced_general_gives_the_stream_kernels_bytes(tmp_path, dtype):
    for mw, mh in STREAM_SHAPES:
        m = matrix_of(mw, mh, 11 * mw + mh)
        src = noise(41, 25, dtype, mw, 131, with_extremes=True, finite=True)
        got = check(tmp_path, src, m, "stream", (mw, mh, name_of(dtype)))
        forced = check(tmp_path, src, m, "general", (mw, mh, name_of(dtype), "forced"), force_general=True)
        same_bits(forced, got, (mw, mh, name_of(dtype), "general against stream"))


# ---------------------------------------------------------------- the general kernel

@pytest.mark.parametrize("shape", [(5, 2), (2, 5), (1, 1), (32, 32)], ids=lambda s: "%dto%d" % s)
def test_general_shapes(tmp_path, shape):
    mw, mh = shape
    m = matrix_of(mw, mh, 13 * mw + mh)
    for dtype in (np.uint8, np.float32):
        for w, h in ((1, 1), (17, 5), (257, 2)):
            src = noise(w, h, dtype, mw, 200 + w, with_extremes=w * h * mw > 16, finite=True)
            check(tmp_path, src, m, "general", (shape, name_of(dtype), w, h))


@pytest.mark.parametrize("dtype", ALL_DTYPES, ids=name_of)
def test_every_format(tmp_path, dtype):
    """3 -> 3 on the one-pel-a-lane kernel, with the format's extremes: float out, double for double."""
    src = noise(17, 5, dtype, 3, 211, with_extremes=True, finite=True)
    m = matrix_of(3, 3, 213)
    got = check(tmp_path, src, m, "general", name_of(dtype), interp=INTERP["srgb"], force_general=True)
    assert got.dtype == (np.float64 if dtype == np.float64 else np.float32)
    streams = dtype in STREAM_DTYPES
    check(tmp_path, src, m, "stream" if streams else "general", (name_of(dtype), "as dispatched"), interp=INTERP["srgb"])


# ---------------------------------------------------------------- cases that catch specific mistakes

@pytest.mark.parametrize("force_general", [False, True], ids=["stream", "general"])
def test_order_and_zeros(tmp_path, force_general):
    kernel = "general" if force_general else "stream"
    # coefficients that are no floats
    check(tmp_path, noise(17, 5, np.uint8, 3, 221, with_extremes=True), SEPIA, kernel, "sepia", INTERP["srgb"], force_general)
    # left to right gives 0, any other order 1
    for dtype in (np.uint8, np.float32):
        got = check(tmp_path, np.ones((3, 5, 3), dtype), [[1e17, 1.0, -1e17]], kernel, "order", INTERP["srgb"], force_general)
        assert (got == 0).all()
    # every product is -0.0: the sum starts at +0.0 and stays there
    got = check(tmp_path, np.zeros((3, 5, 3), np.uint8), [[-1.0, -2.5, -0.1]] * 3, kernel, "negative zeros", INTERP["srgb"], force_general)
    assert not np.signbit(got).any()
    got = check(tmp_path, np.full((3, 5, 1), -0.0, np.float32), [[1.0], [1.0], [1.0]], kernel, "-0.0 times 1", INTERP["b-w"], force_general)
    assert not np.signbit(got).any()


def test_extremes_of_the_wide_formats(tmp_path):
    check(tmp_path, np.full((2, 3, 1), 2 ** 32 - 1, np.uint32), [[0.1]], "general", "uint max")
    check(tmp_path, np.full((2, 3, 1), -2 ** 31, np.int32), [[0.1]], "general", "int min")
    got = check(tmp_path, np.full((2, 3, 1), 2 ** 32 - 1, np.uint32), [[1e35]], "general", "overflow to inf")
    assert np.isposinf(got).all()
    src = noise(17, 5, np.float64, 3, 231, with_extremes=True)
    src.ravel()[20:24] = [np.nan, np.inf, -np.inf, np.nan]
    check(tmp_path, src, matrix_of(3, 3, 233), "general", "double with NaN and inf")
    src = noise(17, 5, np.float32, 3, 235, with_extremes=True)
    src.ravel()[20:24] = [np.nan, np.inf, -np.inf, np.nan]
    check(tmp_path, src, matrix_of(3, 3, 237), "stream", "float with NaN and inf")


@pytest.mark.parametrize("dtype", [np.uint8, np.int32, np.float32, np.float64], ids=name_of)
def test_the_matrix_as_an_image(tmp_path, dtype):
    """vips_check_matrix: a one-band image of any real format, cast to double."""
    m = (matrix_of(3, 3, 241) * 40).astype(dtype) if np.dtype(dtype).kind in "ui" else matrix_of(3, 3, 241).astype(dtype)
    src = noise(17, 5, np.uint8, 3, 243)
    check(tmp_path, src, m, "stream", name_of(dtype), interp=INTERP["srgb"], as_image=True)


def test_refusals(tmp_path):
    im = Image.new_from_array(noise(9, 7, np.uint8, 3, 251), "srgb")
    # more than 32 columns: refused by name, with the size
    wide = Image.new_from_array(noise(5, 4, np.uint8, 33, 253))
    with pytest.raises(VipsHipError, match=r"recomb: a matrix of 33 x 2 is outside the HIP path \(at most 32 x 32\)"):
        wide.recomb(np.ones((2, 33)))
    with pytest.raises(VipsHipError, match=r"recomb: a matrix of 3 x 33 is outside the HIP path"):
        im.recomb(np.ones((33, 3)))
    # the reference's own refusals, in its words
    for m in (np.ones((3, 2)), np.ones((3, 4))):
        with pytest.raises(RuntimeError) as ref:
            ref_recomb(tmp_path, im.numpy(), m)
        with pytest.raises(VipsHipError) as dev:
            im.recomb(m)
        assert str(ref.value).splitlines()[-1].split(": ", 1)[-1] in str(dev.value) and "bands in must equal matrix width" in str(dev.value)
    two_bands = np.ones((3, 3, 2))
    with pytest.raises(RuntimeError) as ref:
        ref_recomb(tmp_path, im.numpy(), two_bands)
    with pytest.raises(VipsHipError) as dev:
        im.recomb(Image.new_from_array(two_bands))
    assert str(ref.value).splitlines()[-1].split(": ", 1)[-1] in str(dev.value) and str(dev.value).startswith("recomb:")
    z = (noise(5, 4, np.float32, 3, 255) + 1j * noise(5, 4, np.float32, 3, 257)).astype(np.complex64)
    with pytest.raises(VipsHipError, match="recomb: image must be non-complex"):
        Image.new_from_array(z).recomb(np.ones((3, 3)))
    with pytest.raises(VipsHipError, match="recomb: image must be non-complex"):
        im.recomb(Image.new_from_array(z[:3, :3, :1]))


# ---------------------------------------------------------------- the capped grid's second turn

def lanes_of_a_step():
    """Runs a stream launch takes before a lane comes back for a second one."""
    return lib.vips_hip_recomb_step(1) * lib.vips_hip_recomb_step(0)


def rows_over_the_grid(width, extra):
    """`extra` more rows than the one-pel-a-lane kernel has in flight for rows of `width` pels."""
    blocks_x = -(-width // lib.vips_hip_recomb_step(0))
    in_flight = -(-lib.vips_hip_recomb_step(1) // blocks_x)
    return blocks_x, in_flight, in_flight + extra


@pytest.mark.parametrize("shape", [(3, 1), (3, 3)], ids=lambda s: "%dto%d" % s)
def test_second_turn_of_the_stream_on_a_whole_image(tmp_path, shape):
    """A whole uchar image (its rows joined) of more runs -- of at most vips_hip_recomb_step(2) pels -- than the grid has
    lanes, the last run ragged: 12 bytes in, one and three 16-byte groups out a run."""
    mw, mh = shape
    run = lib.vips_hip_recomb_step(2)
    side = int(np.sqrt((lanes_of_a_step() + 700) * run + 3)) + 1
    while side * side % run == 0:
        side += 1
    assert side * side // run > lanes_of_a_step()
    src = noise(side, side, np.uint8, mw, 271, with_extremes=True)
    check(tmp_path, src, matrix_of(mw, mh, 273), "stream", ("second turn", shape, side), interp=INTERP["srgb"])


@pytest.mark.parametrize("case", [(np.uint8, (3, 1)), (np.uint16, (3, 3))], ids=lambda c: "%s-%dto%d" % ((name_of(c[0]),) + c[1]))
def test_second_turn_of_the_stream_in_frames(tmp_path, case):
    """Rows that stay rows: a window of a larger frame whose rows together have more runs than the grid has lanes, so
    that the second turn splits its position into a row and a run of it; every row ends in a ragged run, and nothing
    outside the window is written."""
    dtype, (mw, mh) = case
    run = lib.vips_hip_recomb_step(2)
    width = 4096 // (4 * mh) + 1
    runs = -(-width // run)
    height = lanes_of_a_step() // runs + 9
    # (at least ceil(width / most pels of a run) runs a row; the second turn starts inside a row)
    assert width % run and height > 1 and runs * height > lanes_of_a_step() and lanes_of_a_step() % runs
    m = np.ascontiguousarray(matrix_of(mw, mh, 281))
    src = noise(width, height, dtype, mw, 283, with_extremes=True)
    want, _ = ref_recomb(tmp_path, src, m)
    with gated() as g:
        got = gen_in_frames(src, np.float32, mh, lambda i, o: lib.vips_hip_recomb_gen(m.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), mw, mh, i, o), 4)
    assert g.ran == {"recomb_stream": 1}, g.ran
    same_bits(got, want, ("second turn in frames", name_of(dtype), mw, mh))


@pytest.mark.parametrize("case", [(np.uint8, (3, 3), 1, 3), (np.int16, (2, 5), 3, 2), (np.float64, (4, 1), 3, 2)],
                         ids=lambda c: "%s-%dto%d-%dblocks" % ((name_of(c[0]),) + c[1] + (c[2],)))
def test_second_turn_of_the_general_kernel(tmp_path, case):
    """The one-pel-a-lane kernel with more rows than grid.y: rows of one block (grid.y is the cap) and rows of three
    blocks, the last ragged (grid.y is a third of it)."""
    dtype, (mw, mh), blocks, extra = case
    width = (blocks - 1) * lib.vips_hip_recomb_step(0) + 41
    blocks_x, in_flight, rows = rows_over_the_grid(width, extra)
    assert blocks_x == blocks and rows > in_flight and (blocks == 1) == (in_flight == lib.vips_hip_recomb_step(1))
    src = noise(width, rows, dtype, mw, 291, with_extremes=True, finite=True)
    check(tmp_path, src, matrix_of(mw, mh, 293), "general", ("second turn", name_of(dtype), width, rows), force_general=True)


# ---------------------------------------------------------------- the region form

@pytest.mark.parametrize("kernel", ["stream", "general", "unaligned"])
def test_region_form(tmp_path, kernel):
    """Windows cut out of larger frames, whole and strip by strip with strips of one row.  unaligned: rows one element
    off a dword, which the streaming kernel declines for elements smaller than one."""
    margin = 1 if kernel == "unaligned" else 4
    for dtype, (mw, mh) in ((np.uint8, (3, 3)), (np.uint16, (3, 1)), (np.float32, (4, 3)), (np.int16, (2, 5))):
        m = np.ascontiguousarray(matrix_of(mw, mh, 261))
        src = noise(41, 9, dtype, mw, 263, with_extremes=True, finite=True)
        want, _ = ref_recomb(tmp_path, src, m)

        def gen(i, o):
            return lib.vips_hip_recomb_gen(m.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), mw, mh, i, o)

        streams = dtype != np.int16 and (kernel == "stream" or (kernel == "unaligned" and np.dtype(dtype).itemsize >= 4))
        with general_kernel(kernel == "general"), gated() as g:
            got = gen_in_frames(src, np.float32, mh, gen, margin)
        assert g.ran == {"recomb_stream" if streams else "recomb_general": 1}, (name_of(dtype), kernel, g.ran)
        same_bits(got, want, (name_of(dtype), kernel))
        rows = [gen_in_frames(src[y:y + 1], np.float32, mh, gen, margin) for y in range(src.shape[0])]
        same_bits(np.concatenate(rows, axis=0), want, (name_of(dtype), kernel, "strips of one row"))
