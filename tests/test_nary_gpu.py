"""GPU parity: vips_sum and vips_bandrank over arrays of images on the device (libvips_amd/csrc/nary.hip, ops_nary.cpp).

Every comparison is equality of dtype, shape, interpretation and bits against the compiled reference's command line
(`vips sum "a.v b.v c.v" out.v`, `vips bandrank "a.v b.v c.v" out.v --index 1`) -- float and double results as their
integer views; positions where both sides are NaN count as equal.  Nothing has a tolerance: sum adds in the output's
type in index order, bandrank's minimum and maximum are the reference's loops, its other indices are exact for inputs
without NaN (NaN is kept out of those).  Every case asserts by the gate report which of the two kernels ran
(nary_stream, nary_general) and that it was launched once.
Runs on the CPU too, on host fibers (tests/test_emul_arith2.py)."""
import os
import subprocess

import numpy as np
import pytest

import libvips_amd
from libvips_amd import Image, VipsHipError, _ffi
from tests import helpers
from tests.test_arith2_gpu import same_bits
from tests.test_arith_gpu import ALL_DTYPES, noise

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not helpers.have_ref(), reason="oracle/_ref not built")]

lib = _ffi.lib
INTERP = helpers.INTERP
VIPS = os.path.join(helpers.ROOT, "oracle", "_ref", "bin", "vips")
W, H, BANDS = 21, 9, 3  # 567 elements: no multiple of any group of the streaming kernel
KERNELS = ["stream", "general"]


def name_of(dtype):
    return np.dtype(dtype).name


@pytest.fixture(scope="module", autouse=True)
def _init():
    libvips_amd.init(0)


class gated(object):
    """with gated() as g: ...; g.ran: {gate name: launches} of the n-ary kernels that ran inside."""

    def __enter__(self):
        lib.vips_hip_gate_reset()
        lib.vips_hip_gate_enable(1)
        self.ran = None
        return self

    def __exit__(self, *exc):
        try:
            if exc[0] is None:
                self.ran = {k: n for k, (n, _) in libvips_amd.gate_report().items() if k.startswith("nary_")}
        finally:
            lib.vips_hip_gate_enable(0)
            lib.vips_hip_gate_reset()
        return False


class general_kernel(object):
    def __init__(self, on=True):
        self.on = on

    def __enter__(self):
        if self.on:
            os.environ["VIPS_HIP_NO_NARY_STREAM"] = "1"

    def __exit__(self, *exc):
        os.environ.pop("VIPS_HIP_NO_NARY_STREAM", None)
        return False


def ref_cli(tmp_path, op, images, index=None):
    """-> (array, interpretation); RuntimeError with the reference's words.  images: [(array, interpretation)]."""
    paths = []
    for i, (array, interp) in enumerate(images):
        paths.append(str(tmp_path / ("in%d.v" % i)))
        helpers.write_v(paths[-1], array, interp)
    out = str(tmp_path / "out.v")
    cmd = [VIPS, op, " ".join(paths), out] + (["--index", str(index)] if index is not None else [])
    r = subprocess.run(cmd, env=helpers.ref_cli_env(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if r.returncode != 0:
        raise RuntimeError(r.stderr.strip() or "vips %s failed" % op)
    return helpers.read_v(out)


def dev(op, images, index=None):
    ims = [Image.new_from_array(a, i) for a, i in images]
    if op == "sum":
        return Image.sum(ims)
    return ims[0].bandrank(ims[1:]) if index is None else ims[0].bandrank(ims[1:], index=index)


def check(tmp_path, op, images, kernel, what, index=None, ran=None, launches=1):
    want, want_interp = ref_cli(tmp_path, op, images, index)
    with general_kernel(kernel == "general"), gated() as g:
        out = dev(op, images, index)
        got = out.numpy()
    same_bits(got, want, (op, what, kernel, index))
    assert lib.vips_hip_image_get_interpretation(out._h) == want_interp, (op, what)
    # ONE launch, whatever had to be matched
    assert g.ran == ({"nary_" + (ran or kernel): 1} if launches else {}), (op, what, g.ran)
    return got


def array_of(n, dtype, seed, shape=(W, H, BANDS), interp=INTERP["srgb"], extremes=True):
    return [(noise(*shape[:2], dtype, shape[2], seed + 2 * i, with_extremes=extremes and i % 2 == 0, finite=True), interp) for i in range(n)]


# ---------------------------------------------------------------- sum

@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("n", [1, 2, 3, 16])
def test_sum_of_n(tmp_path, n, kernel):
    for dtype in (np.uint8, np.float32):
        check(tmp_path, "sum", array_of(n, dtype, 601), kernel, (n, name_of(dtype)))


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("dtype", ALL_DTYPES, ids=name_of)
def test_sum_formats(tmp_path, dtype, kernel):
    """uint for the unsigned formats, int for the signed ones, float, double.  (int images are kept to a quarter of
    their range: a sum that overflows int is undefined in the reference.)"""
    images = array_of(3, dtype, 611, extremes=dtype != np.int32)
    if dtype == np.int32:
        images = [(a // 4, i) for a, i in images]
    got = check(tmp_path, "sum", images, kernel, name_of(dtype))
    kind = np.dtype(dtype).kind
    assert got.dtype == {"u": np.uint32, "i": np.int32}.get(kind, dtype)


@pytest.mark.parametrize("kernel", KERNELS)
def test_sum_wraps_and_keeps_its_order(tmp_path, kernel):
    # uint wraps
    big = [(np.full((H, W, BANDS), v, np.uint32), INTERP["srgb"]) for v in (2 ** 32 - 1, 2 ** 31, 7)]
    got = check(tmp_path, "sum", big, kernel, "uint wrap")
    assert (got == (2 ** 31 + 6)).all()
    # float order: (1e8f + 1) - 1e8f is 0, any other order gives 1
    order = [(np.full((H, W, BANDS), v, np.float32), INTERP["srgb"]) for v in (1e8, 1.0, -1e8)]
    got = check(tmp_path, "sum", order, kernel, "float order")
    assert (got == 0).all()


def test_sum_matches_formats_bands_and_sizes(tmp_path):
    """vips__formatalike_vec (uchar + short + float is float), vips__bandalike_vec (one band against three, indexed by
    pel) and vips__sizealike_vec (zero outside an image's own rectangle): one launch, no cast but the formats'."""
    mixed = [(noise(W, H, t, BANDS, 621 + i), INTERP["srgb"]) for i, t in enumerate((np.uint8, np.int16, np.float32))]
    assert check(tmp_path, "sum", mixed, "stream", "mixed formats").dtype == np.float32
    bands = [(noise(W, H, np.uint8, b, 631 + i), INTERP["b-w"] if b == 1 else INTERP["srgb"]) for i, b in enumerate((1, 3, 1))]
    check(tmp_path, "sum", bands, "stream", "one band against three", ran="general")
    sizes = [(noise(w, h, np.uint8, 3, 641 + w), INTERP["srgb"]) for w, h in ((7, 5), (4, 9), (6, 6))]
    assert check(tmp_path, "sum", sizes, "stream", "sizes", ran="general").shape == (9, 7, 3)
    with pytest.raises(RuntimeError) as ref:
        ref_cli(tmp_path, "sum", [(noise(5, 4, np.uint8, b, 651), 0) for b in (2, 3)])
    with pytest.raises(VipsHipError) as info:
        dev("sum", [(noise(5, 4, np.uint8, b, 651), 0) for b in (2, 3)])
    assert str(ref.value).splitlines()[-1].split(": ", 1)[-1] in str(info.value) and str(info.value).startswith("sum:")


# ---------------------------------------------------------------- bandrank

@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("n", [1, 2, 3, 5, 16])
def test_bandrank_of_n(tmp_path, n, kernel):
    """The default index (-1: n / 2); one image is a copy, which launches nothing."""
    for dtype in (np.uint8, np.float32):
        check(tmp_path, "bandrank", array_of(n, dtype, 701), kernel, (n, name_of(dtype)), launches=n > 1)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("index", [-1, 0, 1, 2, 3, 4])
def test_bandrank_every_index_of_five(tmp_path, index, kernel):
    base = [a for a, _ in array_of(5, np.uint8, 711)]
    # ties: two images the same, and three rows of one value in three of them
    base[3] = base[1].copy()
    for i in (0, 2, 4):
        base[i][:3] = 77
    for dtype in (np.uint8, np.int16, np.float32):
        shift = 0 if dtype == np.uint8 else 100  # (both signs for the signed formats)
        images = [((a.astype(np.int64) - shift).astype(dtype), INTERP["srgb"]) for a in base]
        check(tmp_path, "bandrank", images, kernel, (name_of(dtype), "ties"), index=index)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("dtype", ALL_DTYPES, ids=name_of)
def test_bandrank_formats(tmp_path, dtype, kernel):
    images = array_of(3, dtype, 721)
    for index in (0, 1, 2):
        got = check(tmp_path, "bandrank", images, kernel, name_of(dtype), index=index)
        assert got.dtype == dtype


@pytest.mark.parametrize("kernel", KERNELS)
def test_bandrank_nan_in_minimum_and_maximum(tmp_path, kernel):
    """bandrank.c:75-105: a NaN in the first image stays (nothing compares below or above it), a NaN later never wins."""
    for dtype in (np.float32, np.float64):
        images = array_of(3, dtype, 731)
        images[0][0].ravel()[10:12] = np.nan
        images[1][0].ravel()[40:42] = np.nan
        images[2][0].ravel()[70:72] = np.nan
        for index in (0, 2):
            got = check(tmp_path, "bandrank", images, kernel, (name_of(dtype), "NaN"), index=index).ravel()
            assert np.isnan(got[10:12]).all() and not np.isnan(got[40:42]).any() and not np.isnan(got[70:72]).any()


def test_bandrank_matches_and_refuses(tmp_path):
    mixed = [(noise(W, H, t, BANDS, 741 + i), INTERP["srgb"]) for i, t in enumerate((np.uint8, np.int16, np.float32))]
    assert check(tmp_path, "bandrank", mixed, "stream", "mixed formats").dtype == np.float32
    bands = [(noise(W, H, np.uint8, b, 751 + i), INTERP["b-w"] if b == 1 else INTERP["srgb"]) for i, b in enumerate((1, 3, 1))]
    check(tmp_path, "bandrank", bands, "stream", "one band against three", ran="general")
    sizes = [(noise(w, h, np.uint8, 3, 761 + w), INTERP["srgb"]) for w, h in ((7, 5), (4, 9), (6, 6))]
    check(tmp_path, "bandrank", sizes, "stream", "sizes", ran="general")
    # index = n is refused in the reference's words
    images = array_of(3, np.uint8, 771)
    with pytest.raises(RuntimeError) as ref:
        ref_cli(tmp_path, "bandrank", images, index=3)
    with pytest.raises(VipsHipError) as info:
        dev("bandrank", images, index=3)
    assert "index out of range" in str(ref.value) and str(info.value).strip() == "bandrank: index out of range"
    z = (noise(5, 4, np.float32, 1, 773) + 1j * noise(5, 4, np.float32, 1, 775)).astype(np.complex64)
    for op in ("sum", "bandrank"):
        with pytest.raises(VipsHipError, match=op + ": image must be non-complex"):
            dev(op, [(z, 0), (z, 0)])


# ---------------------------------------------------------------- the capped grid's second turn

def lanes_of_a_step():
    """Units a stream launch takes before a lane comes back for a second one."""
    return lib.vips_hip_nary_step(1) * lib.vips_hip_nary_step(0)


def side_over_the_grid(unit_elems, bands=BANDS):
    """A square side whose image has 700 more units of `unit_elems` output elements than a capped grid takes in one
    step, and a ragged last unit."""
    elems = (lanes_of_a_step() + 700) * unit_elems + 3
    side = int(np.sqrt(elems // bands)) + 1
    while unit_elems > 1 and side * side * bands % unit_elems == 0:
        side += 1
    assert -(-side * side * bands // unit_elems) > lanes_of_a_step()
    return side


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16], ids=name_of)
def test_sum_second_turn_of_the_stream(tmp_path, dtype):
    """A whole image (its rows joined) of more 16-byte groups of uint than the grid has lanes: the lanes' second unit,
    the last one ragged."""
    side = side_over_the_grid(lib.vips_hip_nary_step(2) // 4)
    images = array_of(3, dtype, 801, shape=(side, side, BANDS))
    assert check(tmp_path, "sum", images, "stream", ("second turn", name_of(dtype))).dtype == np.uint32


@pytest.mark.parametrize("case", [(np.uint8, 1), (np.float64, 1), (np.uint8, 0), (np.int16, 2)], ids=lambda c: "%s-%d" % (name_of(c[0]), c[1]))
def test_bandrank_second_turn_of_the_stream(tmp_path, case):
    """Index 1 of 3 takes a dword (a double) a lane, index 0 and 2 (minimum, maximum) 16 bytes: each over the grid."""
    dtype, index = case
    group = lib.vips_hip_nary_step(2) if index != 1 else lib.vips_hip_nary_step(4 if dtype == np.float64 else 3)
    side = side_over_the_grid(max(1, group // np.dtype(dtype).itemsize))
    images = array_of(3, dtype, 811, shape=(side, side, BANDS))
    check(tmp_path, "bandrank", images, "stream", ("second turn", name_of(dtype)), index=index)


def rows_over_the_grid(elems, extra):
    """`extra` more rows than the one-element-a-lane kernel has in flight for rows of `elems` elements."""
    blocks_x = -(-elems // lib.vips_hip_nary_step(0))
    in_flight = -(-lib.vips_hip_nary_step(1) // blocks_x)
    return blocks_x, in_flight, in_flight + extra


@pytest.mark.parametrize("op", ["sum", "bandrank"])
def test_second_turn_of_the_general_kernel_one_block_a_row(tmp_path, op):
    """Rows of one block, three more of them than grid.y: the blocks' second row."""
    blocks_x, in_flight, rows = rows_over_the_grid(W * BANDS, 3)
    assert blocks_x == 1 and rows > in_flight
    images = array_of(3, np.uint8 if op == "sum" else np.float32, 821, shape=(W, rows, BANDS))
    check(tmp_path, op, images, "general", ("second turn", rows), index=None if op == "sum" else 1)


@pytest.mark.parametrize("op", ["sum", "bandrank"])
def test_second_turn_of_the_general_kernel_three_blocks_a_row(tmp_path, op):
    """Rows of three blocks, the last ragged, two more rows than grid.y (which is not the cap itself here).  The second
    image ends one row into the second turn and the third is narrower: zero outside their own rectangles there too."""
    width = 2 * lib.vips_hip_nary_step(0) // BANDS + 30
    blocks_x, in_flight, rows = rows_over_the_grid(width * BANDS, 2)
    assert blocks_x == 3 and in_flight < lib.vips_hip_nary_step(1) and rows > in_flight and width * BANDS % lib.vips_hip_nary_step(0)
    sizes = [(width, rows), (width, in_flight + 1), (width - 50, rows)]
    images = [(noise(w, h, np.int16, BANDS, 831 + i), INTERP["srgb"]) for i, (w, h) in enumerate(sizes)]
    # (no switch: images of different sizes are the general kernel's as dispatched)
    got = check(tmp_path, op, images, "as dispatched", ("second turn", sizes), index=None if op == "sum" else 0, ran="general")
    assert got.shape == (rows, width, BANDS)


def test_seventeen_images_are_refused_by_name():
    images = [(noise(5, 4, np.uint8, 1, 781 + i), INTERP["b-w"]) for i in range(17)]
    for op in ("sum", "bandrank"):
        with pytest.raises(VipsHipError, match=op + ": arrays of more than 16 images are outside the HIP path"):
            dev(op, images)
