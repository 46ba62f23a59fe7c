"""GPU parity of the exchange kernel's row loop (reduce_fused_u8x4_mfma_x, libvips_amd/csrc/reduce_fused_exch.hip):
batches in which all eight row groups exist and all eight refills are wanted run without a branch around a load
(MfmaStep::batch_steady), a tile's head and rest run the guarded form.  What can go wrong is the seam between the
two, and the replicated edge column of the image's left and right tiles.

With $VIPS_HIP_FUSED_EXCH=1 an image up to 4096 wide gets tiles of 32 output rows: a full tile is 37 groups, the last
row of tiles has oh = out_height mod 32 rows and oh + 5 groups, and the first steady batch needs 12 groups
(MFMA_SLOTS + NB).  The image is 8 * (32 m + oh) rows high: m = 1 walks the ragged row bottom-up, m = 2 top-down.

  oh   groups
   1      6    no whole batch
   3      8    one whole batch, none of whose refills are all wanted
   6     11    one short of the first steady batch
   7     12    exactly the first steady batch
   8     13    one group past it
  11     16    two batches, a short rest
  15 19 27     steady batches followed by rests of different lengths

Every case runs the kernel twice in a row and is checked against the plain-C port and against the kernel with halos
($VIPS_HIP_FUSED_EXCH=0), as tests/test_c2_exchange_gpu.py does.

(Which hand-off a `plain` case runs is the library's to decide: a launch of a few blocks may find a block on another
XCD than its index says, after which the process hands off through memory -- profiles/NOTES.md R8.1.  The row loop
and the edge halo, what these cases are about, are the same code under both.)"""
import functools

import numpy as np
import pytest

import libvips_amd
from libvips_amd import Image
from tests import helpers
from tests.helpers import Port

pytestmark = pytest.mark.gpu

OH = (1, 3, 6, 7, 8, 11, 15, 19, 27)
WIDTHS = (512, 1024, 1536)  # both edges in one tile; a left and a right edge tile; an interior tile between them


@pytest.fixture(scope="module", autouse=True)
def _init():
    libvips_amd.init(0)


@functools.lru_cache(maxsize=None)
def _case(w, h):
    """-> (image, the port's output): made once per shape, shared by the tests, never written to."""
    src = helpers.lcg_image(w, h, 4, np.uint8, 50 + h)
    want = Port.reduce(src, 8, 8, "lanczos3")
    want.setflags(write=False)
    return Image.new_from_array(src), want


def _exchange_twice(im, plain, monkeypatch):
    """-> (first, second) outputs of the exchange kernel, and the kernels that ran."""
    lib = libvips_amd.lib
    monkeypatch.setenv("VIPS_HIP_FUSED_EXCH", "1")
    if not plain:
        monkeypatch.setenv("VIPS_HIP_FUSED_PLAIN", "0")
    lib.vips_hip_gate_reset()
    lib.vips_hip_gate_enable(1)
    try:
        got = im.reduce(8, 8, kernel="lanczos3").numpy()
        again = im.reduce(8, 8, kernel="lanczos3").numpy()
        report = libvips_amd.gate_report()
    finally:
        lib.vips_hip_gate_enable(0)
        lib.vips_hip_gate_reset()
    return got, again, sorted(report)


def _halo_kernel(im, monkeypatch):
    monkeypatch.setenv("VIPS_HIP_FUSED_EXCH", "0")
    try:
        return im.reduce(8, 8, kernel="lanczos3").numpy()
    finally:
        monkeypatch.delenv("VIPS_HIP_FUSED_EXCH")


def _check(w, m, oh, plain, monkeypatch):
    h = 8 * (32 * m + oh)
    im, want = _case(w, h)
    old = _halo_kernel(im, monkeypatch)
    got, again, kernels = _exchange_twice(im, plain, monkeypatch)
    assert kernels == ["reduce_fused_u8_mfma_x"], kernels
    assert got.shape == want.shape
    assert np.array_equal(got, want), (w, h)
    assert np.array_equal(got, old) and np.array_equal(again, got)


@pytest.mark.parametrize("w", WIDTHS)
@pytest.mark.parametrize("oh", OH)
def test_row_loop_seams(oh, w, monkeypatch):
    _check(w, 1, oh, True, monkeypatch)


# the ragged row walked top-down (m = 2), the hand-off through memory: the seam's cases at every width, the longest rest
SUBSET = [(6, 512), (7, 512), (7, 1024), (7, 1536), (8, 1024), (11, 1536), (19, 512), (27, 1536)]


@pytest.mark.parametrize("oh,w", SUBSET)
def test_row_loop_seams_top_down(oh, w, monkeypatch):
    _check(w, 2, oh, True, monkeypatch)


@pytest.mark.parametrize("oh,w", SUBSET)
def test_row_loop_seams_through_memory(oh, w, monkeypatch):
    _check(w, 1, oh, False, monkeypatch)


@pytest.mark.parametrize("w", [512, 1024])
@pytest.mark.parametrize("value", [0, 255])
def test_constant_image_pins_the_edge_column(value, w, monkeypatch):
    """vips_embed(COPY): beyond the image lies its edge column, which the left and right tiles replicate into their
    halos: on a constant image any other byte there shows in the first and last three outputs of every row."""
    h = 8 * (32 + 7)
    src = np.full((h, w, 4), value, np.uint8)
    im = Image.new_from_array(src)
    got, again, kernels = _exchange_twice(im, True, monkeypatch)
    assert kernels == ["reduce_fused_u8_mfma_x"], kernels
    want = Port.reduce(src, 8, 8, "lanczos3")
    assert np.array_equal(got, want) and np.array_equal(again, want)
