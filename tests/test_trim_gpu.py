"""GPU parity: vips_project (combine sum), vips_profile, vips_getpoint and vips_find_trim on the device
(libvips_amd/csrc/trim.hip, ops_trim.cpp).

Everything is np.array_equal on the bytes, with dtype, shape and interpretation, against the compiled reference, which is
reached through its command line on .v files (`vips project in.v c.v r.v`, `vips profile ...`, `vips getpoint in.v x y`,
`vips find_trim in.v --threshold .. --background ".." --line-art`).  Every case asserts by the gate report which kernel
ran and how many launches were made: project one launch, profile one launch, the fused find_trim exactly one trim_fused
(and flatten's launch for an image with alpha) and nothing from rank, arith, logic or project, getpoint none.

Kept out of the inputs, because the reference's answer there is its compiler's or its scheduler's, not its
specification: int images whose column or row sums pass 2^31 (signed overflow; the uint sums that pass 2^32 are in: they
wrap by the C standard); non-integer float and double values in the byte-compared cases (the reference adds per worker
thread and merges in the order its threads stop, project.c:319-361, so only sums that are exact in any order have one
answer: helpers.lcg_image's floats are multiples of 1/256 below 256; the one case of non-integer noise is held to the
bound of any summation order instead); -0.0 in project's float inputs (the first pel a thread meets is assigned, every
other one added, project.c:231-241, so the sign of a zero sum depends on who came first).  Complex images are refused
(getpoint: they stay outside the path).  Runs on the CPU too, on host fibers (tests/test_emul_trim.py)."""
import math
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
ALL_DTYPES = [np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32, np.float32, np.float64]
HISTOGRAM = 10
MULTIBAND, B_W, SRGB = 0, 1, 22
OUT_DTYPES = {"u": np.uint32, "i": np.int32, "f": np.float64}
name_of = lambda d: np.dtype(d).name  # noqa: E731


@pytest.fixture(scope="module", autouse=True)
def _init():
    libvips_amd.init(0)


def step(what):
    return lib.vips_hip_trim_step(what)


class gated(object):
    """with gated() as g: ...; g.report: {gate name: launches} of everything that ran inside."""

    def __enter__(self):
        lib.vips_hip_gate_reset()
        lib.vips_hip_gate_enable(1)
        self.report = None
        return self

    def __exit__(self, *exc):
        try:
            if exc[0] is None:
                self.report = {k: n for k, (n, _) in libvips_amd.gate_report().items()}
        finally:
            lib.vips_hip_gate_enable(0)
            lib.vips_hip_gate_reset()
        return False


class env(object):
    """An environment variable for everything inside (the library reads them at every dispatch)."""

    def __init__(self, name, on=True):
        self.name, self.on = name, on

    def __enter__(self):
        if self.on:
            os.environ[self.name] = "1"

    def __exit__(self, *exc):
        os.environ.pop(self.name, None)
        return False


def same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), what


def run_ref(args):
    r = subprocess.run([VIPS] + args, env=helpers.ref_cli_env(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if r.returncode != 0:
        raise RuntimeError((r.stderr.strip() or "vips %s failed" % args[0]).splitlines()[-1])
    return r.stdout


def ref_pair(tmp_path, op, src, interp=MULTIBAND):
    """-> ((columns, interpretation), (rows, interpretation)) of `vips <op> in.v c.v r.v`."""
    paths = [str(tmp_path / n) for n in ("in.v", "c.v", "r.v")]
    helpers.write_v(paths[0], src, interp)
    run_ref([op] + paths)
    return helpers.read_v(paths[1]), helpers.read_v(paths[2])


def vec(v):
    return " ".join(repr(float(x)) for x in np.atleast_1d(v))


def ref_find_trim(tmp_path, src, interp, threshold=None, background=None, line_art=False):
    path = str(tmp_path / "in.v")
    helpers.write_v(path, src, interp)
    args = ["find_trim", path]
    if threshold is not None:
        args += ["--threshold", repr(float(threshold))]
    if background is not None:
        args += ["--background", vec(background)]
    if line_art:
        args += ["--line-art"]
    return tuple(int(v) for v in run_ref(args).split())


def streams(src):
    """The streaming project kernel takes this (dense) image: 1 .. 4 bands, rows that start on dwords."""
    h, w, b = src.shape
    return b <= 4 and (w * b * src.dtype.itemsize) % 4 == 0


def project_input(w, h, bands, dtype, seed):
    """lcg noise: the whole range for the 8- and 16-bit formats and uint, int kept to 16 bits so that no sum of this file
    passes 2^31, floats multiples of 1/256 below 256."""
    src = helpers.lcg_image(w, h, bands, dtype, seed)
    return src >> 16 if np.dtype(dtype) == np.int32 else src


def profile_input(w, h, bands, dtype, seed):
    """... with all but about one element in 40 zero."""
    keep = helpers.lcg_image(w, h, bands, np.uint8, seed + 1) < 6
    src = helpers.lcg_image(w, h, bands, dtype, seed)
    return np.where(keep, src, 0).astype(dtype)


def check_pair(tmp_path, op, src, what, interp=MULTIBAND, kernels=("stream", "general"), want=None):
    """project or profile of src, under both kernels, against the reference's two images."""
    (wc, wci), (wr, wri) = want or ref_pair(tmp_path, op, src, interp)
    h, w, b = src.shape
    assert wc.shape == (1, w, b) and wr.shape == (h, 1, b) and wci == HISTOGRAM and wri == HISTOGRAM  # (the reference's headers)
    for kernel in kernels:
        with env("VIPS_HIP_NO_TRIM_STREAM", kernel == "general"):
            with gated() as g:
                columns, rows = getattr(Image.new_from_array(src, interp), op)()
                gc, gr = columns.numpy(), rows.numpy()
        same(gc, wc, (op, what, kernel, "columns"))
        same(gr, wr, (op, what, kernel, "rows"))
        for out in (columns, rows):
            assert lib.vips_hip_image_get_interpretation(out._h) == HISTOGRAM
        if op == "profile":
            assert g.report == {"profile": 1}, (what, kernel, g.report)
        else:
            gate = "project_stream" if kernel == "stream" and streams(src) else "project_general"
            assert g.report == {gate: 1}, (what, kernel, g.report)
    return gc, gr


def sweep_sizes(bands, es):
    """1 x 1, 7 x 5, one row, one column, and widths of one block's worth of the streaming kernel's groups - 1 / + 0 / + 1
    pel on more rows than the waves of a block meet after."""
    block = step(0) * step(1) // es  # elements of a row a block of the streaming kernel owns
    sizes = [(1, 1), (7, 5), (61, 1), (1, 37)]
    return sizes + [(max(1, block // bands + d), step(6) + 1) for d in (-1, 0, 1)]


# ---------------------------------------------------------------- project, profile: formats, bands, sizes, both kernels

@pytest.mark.parametrize("bands", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("dtype", ALL_DTYPES, ids=name_of)
def test_project_sweep(dtype, bands, tmp_path):
    for k, (w, h) in enumerate(sweep_sizes(bands, np.dtype(dtype).itemsize)):
        gc, _ = check_pair(tmp_path, "project", project_input(w, h, bands, dtype, 100 + k), (w, h))
        assert gc.dtype == OUT_DTYPES[np.dtype(dtype).kind]  # project.c:99-102


@pytest.mark.parametrize("bands", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("dtype", ALL_DTYPES, ids=name_of)
def test_profile_sweep(dtype, bands, tmp_path):
    for k, (w, h) in enumerate(sweep_sizes(bands, np.dtype(dtype).itemsize)):
        gc, _ = check_pair(tmp_path, "profile", profile_input(w, h, bands, dtype, 200 + k), (w, h), kernels=("stream",))
        assert gc.dtype == np.int32


@pytest.mark.parametrize("bands", [3, 5])
@pytest.mark.parametrize("dtype", [np.uint8, np.int16, np.float32, np.float64], ids=name_of)
def test_over_the_grid(dtype, bands, tmp_path):
    """A few more rows than a capped grid takes in one step (a lane's second step, the sums across the blocks, the last
    tile ragged), one block wide: an element size each, the streaming kernel (3 bands) and the general one (5)."""
    w, h = 8, step(3) * step(6) + 2 * step(6) + 3
    check_pair(tmp_path, "project", project_input(w, h, bands, dtype, 301), (w, h), kernels=("stream",))
    check_pair(tmp_path, "profile", profile_input(w, h, bands, dtype, 302), (w, h), kernels=("stream",))


def test_project_interpretation_and_windows(tmp_path):
    """The outputs are histograms whatever the input was tagged; rows that do not start on dwords (a 3-band uchar image
    of odd width) go one element a lane."""
    src = project_input(33, 9, 3, np.uint8, 310)
    assert not streams(src)
    check_pair(tmp_path, "project", src, "odd rows", interp=SRGB)
    check_pair(tmp_path, "profile", profile_input(33, 9, 3, np.uint8, 311), "odd rows", interp=SRGB)


# ---------------------------------------------------------------- project: wrapping and ranges

def test_project_uint_wraps(tmp_path):
    """uint sums that pass 2^32 wrap, as the C standard says of the reference's guint accumulators."""
    src = helpers.lcg_image(37, 45, 3, np.uint32, 320) | np.uint32(0x80000000)
    gc, gr = check_pair(tmp_path, "project", src, "wrap")
    assert src.astype(np.uint64).sum(axis=0).max() > 2 ** 32 and src.astype(np.uint64).sum(axis=1).max() > 2 ** 32
    assert np.array_equal(gc[0], (src.astype(np.uint64).sum(axis=0) & 0xFFFFFFFF).astype(np.uint32))


@pytest.mark.parametrize("dtype", [np.uint16, np.int16], ids=name_of)
def test_project_16_bit_noise(dtype, tmp_path):
    rng = np.random.default_rng(330)
    info = np.iinfo(dtype)
    src = rng.integers(info.min, info.max, (150, 519, 2), dtype=dtype, endpoint=True)
    src[0, 0], src[-1, -1] = info.min, info.max
    check_pair(tmp_path, "project", np.ascontiguousarray(src), "noise")


@pytest.mark.parametrize("kernel", ["stream", "general"])
def test_project_float_sums(kernel):
    """Non-integer noise: every sum against math.fsum of the same values within (N - 1) * 2^-53 * sum|x|, N the terms of
    that sum: the bound of any double summation order, which the reference meets as the device does; the same image
    twice gives the same bits."""
    rng = np.random.default_rng(340)
    src = ((rng.random((67, 1031, 3)) - 0.5) * 600.0).astype(np.float32)
    with env("VIPS_HIP_NO_TRIM_STREAM", kernel == "general"):
        im = Image.new_from_array(src)
        (c1, r1), (c2, r2) = im.project(), im.project()
        c1, r1, c2, r2 = c1.numpy(), r1.numpy(), c2.numpy(), r2.numpy()
    assert np.array_equal(c1.view(np.uint64), c2.view(np.uint64)) and np.array_equal(r1.view(np.uint64), r2.view(np.uint64))
    u = 2.0 ** -53
    v = src.astype(np.float64)
    h, w, b = src.shape
    for x in range(w):
        for k in range(b):
            assert abs(c1[0, x, k] - math.fsum(v[:, x, k])) <= (h - 1) * u * math.fsum(np.abs(v[:, x, k])), (x, k)
    for y in range(h):
        for k in range(b):
            assert abs(r1[y, 0, k] - math.fsum(v[y, :, k])) <= (w - 1) * u * math.fsum(np.abs(v[y, :, k])), (y, k)


def test_project_profile_refuse_complex(tmp_path):
    src = np.zeros((3, 4, 1), np.complex64)
    for op in ("project", "profile"):
        with pytest.raises(RuntimeError) as ref:
            ref_pair(tmp_path, op, src)
        with pytest.raises(VipsHipError) as info:
            getattr(Image.new_from_array(src), op)()
        assert str(info.value).strip() == str(ref.value) == "%s: image must be non-complex" % op


# ---------------------------------------------------------------- profile: edge cases

def test_profile_edges(tmp_path):
    """All zero; a single non-zero element at each corner and either side of a block's boundary (columns) and of a
    meeting of the block's waves (rows)."""
    w, h = step(0) + 9, step(6) + 5
    zero = np.zeros((h, w, 2), np.uint8)
    gc, gr = check_pair(tmp_path, "profile", zero, "all zero", kernels=("stream",))
    assert (gc == h).all() and (gr == w).all()
    spots = [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (step(0) - 1, 3), (step(0), 3), (5, step(6) - 1), (5, step(6)),
             (63, 2), (64, 2)]
    for x, y in spots:
        for band in (0, 1):
            src = zero.copy()
            src[y, x, band] = 1
            gc, gr = check_pair(tmp_path, "profile", src, (x, y, band), kernels=("stream",))
            assert gc[0, x, band] == y and gr[y, 0, band] == x and (gc == h).sum() == gc.size - 1


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=name_of)
def test_profile_nan_and_negative_zero(dtype, tmp_path):
    """C's `if (p[j])`: a NaN counts, -0.0 does not."""
    src = np.zeros((6, 9, 1), dtype)
    src[1, 2], src[3, 4], src[4, 4], src[5, 8] = -0.0, np.nan, 1.0, -0.0
    gc, gr = check_pair(tmp_path, "profile", src, "nan")
    assert gc[0, 4, 0] == 3 and gr[3, 0, 0] == 4 and gc[0, 2, 0] == 6 and gr[1, 0, 0] == 9 and gr[5, 0, 0] == 9


# ---------------------------------------------------------------- getpoint

@pytest.mark.parametrize("bands", [1, 5])
@pytest.mark.parametrize("dtype", ALL_DTYPES, ids=name_of)
def test_getpoint(dtype, bands, tmp_path):
    src = helpers.lcg_image(11, 7, bands, dtype, 400)
    if np.dtype(dtype).kind == "f":
        src = (src / 7).astype(dtype)  # (not short decimals)
    path = str(tmp_path / "in.v")
    helpers.write_v(path, src)
    im = Image.new_from_array(src)
    for x, y in ((0, 0), (10, 6), (3, 5)):
        want = [float(v) for v in run_ref(["getpoint", path, str(x), str(y)]).split()]
        with gated() as g:
            got = im.getpoint(x, y)
        assert got == want == [float(v) for v in src[y, x]], (x, y)
        assert g.report == {}  # a copy of the pel: no launch
    for x, y in ((11, 0), (0, 7)):
        with pytest.raises(RuntimeError) as ref:
            run_ref(["getpoint", path, str(x), str(y)])
        with pytest.raises(VipsHipError) as info:
            im.getpoint(x, y)
        assert str(info.value).strip() == str(ref.value) == "extract_area: bad extract area"
    # (the command line takes -1 for an option; vips_crop refuses it in the same words)
    for x, y in ((-1, 0), (0, -1)):
        with pytest.raises(VipsHipError, match="extract_area: bad extract area"):
            im.getpoint(x, y)


def test_getpoint_refuses_complex():
    with pytest.raises(VipsHipError, match="outside the HIP path"):
        Image.new_from_array(np.zeros((2, 2, 1), np.complex64)).getpoint(0, 0)


# ---------------------------------------------------------------- find_trim: both routes against the reference

FLATTEN_GATES = {"flatten_u8", "flatten_any"}


def fused_takes(src, interp, background):
    """The one-launch route takes this image: uchar, 1 .. 4 bands after the flatten, a background of 1 or that many."""
    bands = src.shape[2]
    base = {B_W: 1, SRGB: 3}.get(interp, 0)
    after = bands - 1 if base and bands > base else bands
    n = 1 if background is None else len(np.atleast_1d(background))
    return src.dtype == np.uint8 and after <= 4 and n in (1, after), after != bands


def check_find_trim(tmp_path, src, interp, what, **options):
    """Both routes against the reference's four numbers, or all three an error in the same words."""
    opts = {k: v for k, v in options.items() if v is not None}
    try:
        want = ref_find_trim(tmp_path, src, interp, **opts)
    except RuntimeError as e:
        for composed in (False, True):
            with env("VIPS_HIP_NO_TRIM_FUSED", composed):
                with pytest.raises(VipsHipError) as info:
                    Image.new_from_array(src, interp).find_trim(**opts)
            assert str(info.value).strip() == str(e), (what, options, composed)
        return None
    takes, alpha = fused_takes(src, interp, opts.get("background"))
    for composed in (False, True):
        with env("VIPS_HIP_NO_TRIM_FUSED", composed):
            with gated() as g:
                got = Image.new_from_array(src, interp).find_trim(**opts)
        assert got == want, (what, options, "composed" if composed else "fused", got, want)
        flattens = sum(n for k, n in g.report.items() if k in FLATTEN_GATES)
        assert flattens == (1 if alpha else 0), (what, g.report)
        rest = {k: n for k, n in g.report.items() if k not in FLATTEN_GATES and k != "cast"}
        if takes and not composed:
            # ONE launch over the image: nothing from rank, arith, logic or project
            assert rest == {"trim_fused": 1}, (what, options, g.report)
        else:
            assert "trim_fused" not in rest and sum(n for k, n in rest.items() if k.startswith("project_")) == 1, (what, g.report)
            assert sum(n for k, n in rest.items() if k.startswith("rank_")) == (0 if opts.get("line_art") else 1), (what, g.report)
    return want


def canvas(w, h, bands, value=255):
    return np.full((h, w, bands), value, np.uint8)


def with_object(w, h, bands, left, top, ow, oh, value=40):
    src = canvas(w, h, bands)
    src[top:top + oh, left:left + ow] = value
    return src


@pytest.mark.parametrize("line_art", [False, True], ids=["median", "line_art"])
@pytest.mark.parametrize("size", [(1, 1), (1, 9), (9, 1), (2, 2)], ids=str)
def test_find_trim_tiny(size, line_art, tmp_path):
    """Images smaller than the median's window: the reference refuses them in vips_rank's words unless line_art."""
    w, h = size
    for bands in (1, 3):
        src = canvas(w, h, bands)
        src[h - 1, w - 1] = 0
        check_find_trim(tmp_path, src, MULTIBAND, size, line_art=line_art)


def tile_sizes(bands):
    """Widths and heights round a fused tile (its row is step(4) elements, it is step(2) rows high) and round the rows a
    fused block takes, - 1 / + 0 / + 1."""
    tw = -(-step(4) // bands)
    return [(tw + d, step(2) + d) for d in (-1, 0, 1)] + [(2 * tw + d, step(5) + d) for d in (-1, 0, 1)]


@pytest.mark.parametrize("bands", [1, 3, 4])
def test_find_trim_contents(bands, tmp_path):
    """Nothing above the threshold, everything above it, an object that touches each edge and each tile boundary."""
    for w, h in tile_sizes(bands):
        check_find_trim(tmp_path, canvas(w, h, bands), MULTIBAND, ("nothing", w, h))
        check_find_trim(tmp_path, canvas(w, h, bands, 3), MULTIBAND, ("everything", w, h))
    tw, th, bh = -(-step(4) // bands), step(2), step(5)
    w, h = 2 * tw + 1, bh + 9
    boxes = [(0, 0, 5, 4), (w - 6, 0, 6, 5), (0, h - 4, 7, 4), (w - 5, h - 5, 5, 5),       # the corners and edges
             (tw - 4, th - 4, 4, 4), (tw, th, 4, 4), (tw - 2, th - 2, 5, 5),                # round a tile's corner
             (tw - 3, bh - 3, 3, 3), (tw, bh, 4, 3), (3, bh - 2, w - 6, 4), (0, 0, w, h)]   # round a block's last row
    for box in boxes:
        want = check_find_trim(tmp_path, with_object(w, h, bands, *box), MULTIBAND, box)
        assert want == box, (box, want)  # (objects of 3 x 3 and more with straight edges pass the median whole)


@pytest.mark.parametrize("bands", [1, 3])
def test_find_trim_specks(bands, tmp_path):
    """A single pel and a 2 x 2 speck: the median removes them, line_art keeps them."""
    w, h = 41, 23
    for box in ((17, 9, 1, 1), (30, 15, 2, 2)):
        src = with_object(w, h, bands, *box)
        assert check_find_trim(tmp_path, src, MULTIBAND, box) == (w, h, 0, 0)
        assert check_find_trim(tmp_path, src, MULTIBAND, box, line_art=True) == box
    # ... in the image's corners, where the copied edge counts the speck several times
    for box in ((0, 0, 1, 1), (w - 2, h - 2, 2, 2), (w - 1, 0, 1, 2)):
        src = with_object(w, h, bands, *box)
        check_find_trim(tmp_path, src, MULTIBAND, box)
        assert check_find_trim(tmp_path, src, MULTIBAND, box, line_art=True) == box
    # a line on the image's last row, an odd height: the row a lane would make below it is no row of the image
    assert check_find_trim(tmp_path, with_object(w, h, bands, 10, h - 1, 3, 1), MULTIBAND, "last row") == (11, h - 1, 1, 1)
    # one band alone differs: the OR across the bands
    if bands == 3:
        src = canvas(w, h, bands)
        src[5:11, 7:19, 1] = 100
        assert check_find_trim(tmp_path, src, MULTIBAND, "one band") == (7, 5, 12, 6)


@pytest.mark.parametrize("threshold", [10, 0, 0.5, -1, 300])
@pytest.mark.parametrize("background", [None, 255, 0, "vector", 127.5], ids=str)
def test_find_trim_options(background, threshold, tmp_path):
    """Backgrounds 255, 0, a vector and 127.5, thresholds 10, 0, 0.5, -1 (outside the property's range: the reference
    leaves the default in place) and 300 (nothing passes), on noise round the background and on a soft-edged object."""
    for bands in (1, 3):
        bg = [250.0, 3.5, 128.0][:bands] if background == "vector" else background
        w, h = 57, 31
        centre = np.atleast_1d(255 if bg is None else bg).astype(np.float64)
        centre = np.resize(centre, bands)
        noise = helpers.lcg_image(w, h, bands, np.uint8, 500 + bands).astype(np.int32) % 25 - 12
        src = np.clip(np.rint(centre)[None, None, :] + noise, 0, 255).astype(np.uint8)
        src[9:20, 13:40] = np.clip(src[9:20, 13:40].astype(np.int32) - 90, 0, 255).astype(np.uint8) if centre[0] > 100 else 200
        for line_art in (False, True):
            check_find_trim(tmp_path, src, MULTIBAND, (bands, bg), threshold=threshold, background=bg, line_art=line_art)


def test_find_trim_background_length(tmp_path):
    """A background whose length vips_linear refuses: its error, word for word, on both routes; a vector against a
    one-band image is banded up (the composed route alone takes it)."""
    check_find_trim(tmp_path, canvas(9, 9, 3), MULTIBAND, "two of three", background=[1, 2])
    check_find_trim(tmp_path, canvas(9, 9, 4), MULTIBAND, "three of four", background=[1, 2, 3], line_art=True)
    src = canvas(12, 10, 1, 0)
    src[3:8, 2:9] = 2
    check_find_trim(tmp_path, src, B_W, "banded up", background=[0, 1, 2], threshold=0.5, line_art=True)
    check_find_trim(tmp_path, src, B_W, "banded up", background=[0, 1, 2], threshold=0.5)


@pytest.mark.parametrize("case", ["rgba", "grey_alpha"])
def test_find_trim_alpha(case, tmp_path):
    """RGBA and grey + alpha go through the flatten against the background, then the same two routes."""
    bands, interp = (4, SRGB) if case == "rgba" else (2, B_W)
    w, h = -(-step(4) // (bands - 1)) + 3, step(2) * 2 + 1
    src = helpers.lcg_image(w, h, bands, np.uint8, 600)
    src[..., -1] = 0           # transparent: the background shows
    src[4:13, 6:w - 9, -1] = 255  # an opaque object of noise
    src[4:13, 6:w - 9, :-1] //= 2
    src[1, 1, -1] = 90         # a translucent speck
    for background in (None, 0, [10, 200, 30][:bands - 1]):
        for line_art in (False, True):
            check_find_trim(tmp_path, src, interp, (case, background), background=background, line_art=line_art)
    # default background by interpretation, no alpha: multiband 4 bands is four colour bands
    check_find_trim(tmp_path, src, MULTIBAND, (case, "no alpha"))


@pytest.mark.parametrize("dtype", [np.uint16, np.float32], ids=name_of)
def test_find_trim_composed_formats(dtype, tmp_path):
    """ushort and float images take the composed route whatever is asked for."""
    w, h = 47, 29
    interp = 25 if dtype == np.uint16 else MULTIBAND  # RGB16: the default background is 65535
    white = 65535 if dtype == np.uint16 else 255
    src = np.full((h, w, 3), white, dtype)
    src[6:17, 9:33] = (white // 3)
    src[20, 40] = 0
    assert check_find_trim(tmp_path, src, interp, name_of(dtype)) == (9, 6, 24, 11)
    assert check_find_trim(tmp_path, src, interp, name_of(dtype), line_art=True, threshold=100.5) == (9, 6, 32, 15)


# ---------------------------------------------------------------- the predicate table, whole domain

TABLE_PAIRS = [(255, 10), (0, 10), (127.5, 0), (127.5, 0.5), (128, 0), (100.25, 27.75), (-20, 30), (300, 60.5), (255, 254.5),
               (0, 255), (3.999, 0.001), (200, 1e-9), (17, 1e9)]


@pytest.mark.parametrize("bands", [1, 3, 4])
def test_find_trim_table_whole_domain(bands, tmp_path):
    """A 256 x 1 image holding every byte value in every band, line_art on: for (background, threshold) pairs with
    fractional and out-of-range values the fused answer (the host-made table) equals the composed chain's and both equal
    the reference's.  With a vector background every band has a table of its own."""
    ramp = np.arange(256, dtype=np.uint8)
    src = np.stack([np.roll(ramp, 37 * k) for k in range(bands)], axis=1)[None]
    for bg, threshold in TABLE_PAIRS:
        check_find_trim(tmp_path, src, MULTIBAND, (bg, threshold), background=bg, threshold=threshold, line_art=True)
        vector = [bg, bg / 2 + 1.25, 255 - bg, 31.5][:bands]
        check_find_trim(tmp_path, src, MULTIBAND, (vector, threshold), background=vector, threshold=threshold, line_art=True)
        # one column per value, so that the left and right bounds single out the first and last value that pass
        check_find_trim(tmp_path, np.ascontiguousarray(src[:, ::-1]), MULTIBAND, (bg, threshold, "reversed"), background=bg,
                        threshold=threshold, line_art=True)
