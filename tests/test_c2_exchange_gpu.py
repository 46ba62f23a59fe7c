"""GPU parity of the exchange kernel (reduce_fused_u8x4_mfma_x: vips_reduce(8, 8, lanczos3) on RGBA uchar, a tile
512 aligned columns wide, the outputs straddling a tile boundary made as partial sums by both tiles and finished by
the later one) in its one-pass horizontal walk: eight segments of nine outputs make a tile's 64 outputs and the
three straddling ones either side.  Every case runs the kernel twice in a row (the arrival counters live on) in both
hand-off forms (through the XCD's L2, and write-through: $VIPS_HIP_FUSED_PLAIN=0), and is checked against the
plain-C port and against the kernel with halos ($VIPS_HIP_FUSED_EXCH=0)."""
import numpy as np
import pytest

import libvips_amd
from libvips_amd import Image
from tests import helpers
from tests.helpers import Port

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _init():
    libvips_amd.init(0)


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


# (width, height): tiles of 32 output rows (the least), tiles_x x tiles_y, the last row of tiles ragged:
#   512 x 808    one tile wide (both sides the image's edge), 4 rows of tiles, the last (bottom-up) 5 rows
#   1024 x 568   2 x 3, the last row (top-down) 7 rows
#   1536 x 520   3 x 3, the last row (top-down) 1 row
#   2048 x 1016  4 x 4, the last row (bottom-up) 31 rows
#   512 x 256    one tile, whole
@pytest.mark.parametrize("plain", [True, False])
@pytest.mark.parametrize("size", [(512, 808), (1024, 568), (1536, 520), (2048, 1016), (512, 256)])
def test_exchange_ragged_tiles(size, plain, monkeypatch):
    w, h = size
    src = helpers.lcg_image(w, h, 4, np.uint8, 50)
    im = Image.new_from_array(src)
    old = _halo_kernel(im, monkeypatch)
    got, again, kernels = _exchange_twice(im, plain, monkeypatch)
    assert kernels == ["reduce_fused_u8_mfma_x"], kernels
    want = Port.reduce(src, 8, 8, "lanczos3")
    assert got.shape == want.shape
    assert np.array_equal(got, want), str(size)
    assert np.array_equal(got, old) and np.array_equal(again, old)


def _bands_vs_port(src_dev, got, rows=48):
    """The port on the image's first and last 8 * (rows + 8) input rows (all columns: every tile boundary), compared
    on the output rows that band's clamped edge does not reach."""
    h = src_dev.shape[0]
    band = 8 * (rows + 8)
    top = Port.reduce(src_dev[:band].cpu().numpy(), 8, 8, "lanczos3")
    assert np.array_equal(got[:rows], top[:rows])
    bottom = Port.reduce(src_dev[h - band:].cpu().numpy(), 8, 8, "lanczos3")
    assert np.array_equal(got[-rows:], bottom[-rows:])


# Tiles of 128 output rows (the most) take ~1 GiB inputs, one residency round of tiles:
#   16384 x 16360  32 x 16 tiles, the last row (bottom-up) 125 rows
#   12288 x 21464  24 x 21 tiles, the last row (top-down) 123 rows
@pytest.mark.parametrize("plain", [True, False])
@pytest.mark.parametrize("size", [(16384, 16360), (12288, 21464)])
def test_exchange_c2_full_oht128(size, plain, monkeypatch):
    import torch

    from bench import lcg_image_device

    w, h = size
    src = lcg_image_device(torch, w, h, 4, 777, torch.device("cuda", 0))
    torch.cuda.synchronize()
    im = Image.new_from_tensor(src)
    old = _halo_kernel(im, monkeypatch)
    got, again, kernels = _exchange_twice(im, plain, monkeypatch)
    assert kernels == ["reduce_fused_u8_mfma_x"], kernels
    assert got.shape == (h // 8, w // 8, 4)
    assert np.array_equal(got, old) and np.array_equal(again, old)
    _bands_vs_port(src, got)
