"""Speed of the rot / flip kernels (libvips_amd/csrc/rot.hip) on images beyond the Infinity Cache: every angle and
both flips, gate (event) timing, 5 warm-up and 20 timed calls; beside each, two yardsticks measured in the same
process -- a device-to-device copy of the same bytes (vips_hip_memcpy_d2d) and cast uchar -> ushort on the same number
of elements -- and the reference's rot d90 on the host cores.  GB/s are over the algorithmic bytes: the image read
once and written once.  Usage: time_rot.py [output file]   (ROT_PERF_SCALE=4 shrinks every side, for a rehearsal)"""
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

SCALE = int(os.environ.get("ROT_PERF_SCALE", "1"))
WARM, TIMED = 5, 20
lib = _ffi.lib
libvips_amd.init(0)
rng = np.random.default_rng(11)
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def timed(fn):
    """-> {gate: (launches, ms)} of TIMED calls after WARM."""
    for _ in range(WARM):
        fn()
    libvips_amd.synchronize()
    lib.vips_hip_gate_reset()
    lib.vips_hip_gate_enable(1)
    try:
        for _ in range(TIMED):
            fn()
        libvips_amd.synchronize()
        return libvips_amd.gate_report()
    finally:
        lib.vips_hip_gate_enable(0)
        lib.vips_hip_gate_reset()


def copy_ms(im, nbytes):
    """A device-to-device copy of the image's bytes, host clock round a window that ends in a synchronise."""
    dst = lib.vips_hip_malloc(nbytes)
    assert dst
    try:
        for _ in range(WARM):
            _ffi.check(lib.vips_hip_memcpy_d2d(dst, im.data_ptr, nbytes))
        libvips_amd.synchronize()
        t0 = time.perf_counter()
        for _ in range(TIMED):
            _ffi.check(lib.vips_hip_memcpy_d2d(dst, im.data_ptr, nbytes))
        libvips_amd.synchronize()
        return (time.perf_counter() - t0) * 1e3 / TIMED
    finally:
        lib.vips_hip_free(dst)


def cast_ms(width, height, bands):
    """cast uchar -> ushort on as many elements: the project's yardstick for pure movement (3 bytes an element)."""
    im = Image.new_from_array(rng.integers(0, 256, size=(height, width, bands), dtype=np.uint8))
    report = timed(lambda: im.cast("ushort"))
    return max(sum(ms for _, ms in report.values()) / TIMED, 1e-9)


IMAGES = [(8192, 8192, 3, np.uint8), (16384, 16384, 4, np.uint8), (8192, 8192, 3, np.float32)]
OPS = [("rot d90", lambda im: im.rot("d90")), ("rot d180", lambda im: im.rot("d180")), ("rot d270", lambda im: im.rot("d270")),
       ("flip horizontal", lambda im: im.flip("horizontal")), ("flip vertical", lambda im: im.flip("vertical"))]

say("# %d warm-up + %d timed calls; kernels: gate (event) timing; copy: host clock round %d copies and a synchronise" % (WARM, TIMED, TIMED))
say("# GB/s over the algorithmic bytes (the image read once, written once); 'of copy' = copy ms / kernel ms")
for width, height, bands, dtype in IMAGES:
    width, height = width // SCALE, height // SCALE
    if np.dtype(dtype).kind == "f":
        src = rng.random(size=(height, width, bands), dtype=np.float32)
    else:
        src = rng.integers(0, 256, size=(height, width, bands), dtype=dtype)
    nbytes = src.nbytes
    im = Image.new_from_array(src)
    c_ms = copy_ms(im, nbytes)
    k_ms = cast_ms(width, height, bands)
    elements = width * height * bands
    say("")
    say("## %d x %d x %d %s (%.0f MB)" % (width, height, bands, np.dtype(dtype).name, nbytes / 1e6))
    say("  %-16s %-22s %9s %9s %8s" % ("operation", "kernel(s)", "ms", "GB/s", "of copy"))
    say("  %-16s %-22s %9.3f %9.1f %8s" % ("copy d2d", "vips_hip_memcpy_d2d", c_ms, 2 * nbytes / c_ms / 1e6, "1.00"))
    say("  %-16s %-22s %9.3f %9.1f %8.2f   (%d elements, 3 bytes each)" % (
        "cast u8->u16", "cast", k_ms, 3 * elements / k_ms / 1e6, c_ms / k_ms, elements))
    for name, op in OPS:
        report = timed(lambda: op(im))
        assert all(n == TIMED for n, _ in report.values()), report
        ms = max(sum(t for _, t in report.values()) / TIMED, 1e-9)
        say("  %-16s %-22s %9.3f %9.1f %8.2f" % (name, "+".join(sorted(report)), ms, 2 * nbytes / ms / 1e6, c_ms / ms))
    if helpers.have_ref():
        ref_s = Ref.time_chain("rot:angle=d90", src, repeats=2)
        say("  %-16s %-22s %9.1f %9.1f %8s   (%d threads)" % ("rot d90", "reference, host cores", ref_s * 1e3,
                                                           2 * nbytes / ref_s / 1e9, "", Ref.concurrency()))
    del im, src
say("PERF-OK")
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
