"""Speed of the one-launch grey kernels on 16384 x 16384 images (beyond the Infinity Cache), gate timing,
5 warm-up and 20 timed calls; cast uchar -> ushort beside them as the yardstick; the reference on the host."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import libvips_amd  # noqa: E402
from libvips_amd import Image, _ffi  # noqa: E402
from tests import helpers  # noqa: E402
from tests.helpers import Ref  # noqa: E402

N = int(os.environ.get("MONO_PERF_SIZE", "16384"))
WARM, TIMED = 5, 20
PEAK = 8e12
INTERP = {"b-w": 1, "srgb": 22, "rgb16": 25, "grey16": 26}
lib = _ffi.lib
libvips_amd.init(0)
rng = np.random.default_rng(7)


def image(bands, dtype):
    info = np.iinfo(dtype)
    return rng.integers(0, info.max + 1, size=(N, N, bands), dtype=dtype)


def timed(fn):
    for _ in range(WARM):
        fn()
    libvips_amd.synchronize()
    lib.vips_hip_gate_reset()
    lib.vips_hip_gate_enable(1)
    try:
        for _ in range(TIMED):
            fn()
        libvips_amd.synchronize()
        report = libvips_amd.gate_report()
    finally:
        lib.vips_hip_gate_enable(0)
        lib.vips_hip_gate_reset()
    return report


CASES = [("srgb", "b-w", 3, np.uint8, 3 + 1), ("srgb", "grey16", 3, np.uint8, 3 + 2), ("rgb16", "b-w", 3, np.uint16, 6 + 1),
         ("b-w", "grey16", 1, np.uint8, 1 + 2), ("grey16", "b-w", 1, np.uint16, 2 + 1)]
print("# %d x %d pixels, %d warm-up + %d timed calls, gate (event) timing; GB/s over the algorithmic bytes" % (N, N, WARM, TIMED))
print("# %-18s %-18s %9s %9s %7s %12s" % ("operation", "kernel", "ms", "GB/s", "of 8TB/s", "reference ms"))
rows = []
for a, b, bands, dtype, bpp in CASES:
    src = image(bands, dtype)
    im = Image.new_from_array(src, interpretation=a)
    report = timed(lambda: im.colourspace(b))
    assert len(report) == 1, report
    (kernel, (launches, total_ms)), = report.items()
    assert launches == TIMED, report
    ms = max(total_ms / launches, 1e-9)
    gbs = N * N * bpp / (ms * 1e-3) / 1e9
    t0 = time.time()
    ref_s = Ref.time_chain("colourspace:space=" + b, src, repeats=3, interpretation=INTERP[a])
    rows.append((a, b, kernel, ms, gbs, ref_s))
    print("  %-18s %-18s %9.3f %9.1f %6.1f%% %12.1f   (reference: %d threads)" % (
        a + " -> " + b, kernel, ms, gbs, 100 * gbs * 1e9 / PEAK, ref_s * 1e3, Ref.concurrency()), flush=True)
    del im, src
src = image(1, np.uint8)
im = Image.new_from_array(src)
report = timed(lambda: im.cast("ushort"))
for kernel, (launches, total_ms) in report.items():
    ms = max(total_ms / launches, 1e-9)
    gbs = N * N * 3 / (ms * 1e-3) / 1e9
    print("  %-18s %-18s %9.3f %9.1f %6.1f%%" % ("cast uchar->ushort", kernel, ms, gbs, 100 * gbs * 1e9 / PEAK))
print("PERF-OK")
