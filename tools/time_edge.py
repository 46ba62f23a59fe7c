"""What the edge detectors cost (libvips_amd/csrc/edge.hip), on an 8192 x 8192 x 3 uchar image, every case in ONE
process on one device:

  * the yardstick: one integer 3 x 3 convolution of the same image (scale 2, offset 128: the convolution sobel runs
    twice), and two of them -- what the image would cost before the combine if the masks ran one after the other;
    beside it a 3 x 3 convolution with scale 1 and no offset, which the matrix-core kernel of conv_u8_mfma.hip takes;
  * sobel, scharr and prewitt on the fused kernel; sobel through the general tier (the Highway arithmetic of convi
    selected: two convolutions and the uchar combine), and on a float image (two float convolutions and the combine);
  * compass, times = 8, angle d45, max and sum, on the fused kernel, against eight convolutions;
  * canny at sigma 1.4 in both precisions, each beside the gaussblur it starts with: the difference is the fused tail.

Each case reports: ms a call (device events on the library's stream round TIMED calls after WARM), the algorithmic
bytes (input + output, once each) over that time as a fraction of 8 TB/s, the ratio to the yardstick, and the kernels
that ran (gate report).
Usage: time_edge.py [output file]   (EDGE_PERF_SCALE=8 shrinks every side, for a rehearsal)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCALE = int(os.environ.get("EDGE_PERF_SCALE", "1"))
SIDE = 8192 // SCALE
BANDS = 3
WARM, TIMED = 3, 10
PEAK = 8e12

SOBEL = np.array([[1.0, 2.0, 1.0], [0.0, 0.0, 0.0], [-1.0, -2.0, -1.0]])
SOBEL90 = np.ascontiguousarray(np.rot90(SOBEL, -1))
KIRSCH = np.array([[5.0, 5.0, 5.0], [-3.0, 0.0, -3.0], [-3.0, -3.0, -3.0]])


def main():
    import libvips_amd
    from libvips_amd import Image, _ffi
    from tests import helpers

    lib = _ffi.lib
    libvips_amd.init(0)
    src = helpers.lcg_image(SIDE, SIDE, BANDS, np.uint8, 5)
    im = Image.new_from_array(src)
    imf = im.cast("float")
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def conv1(mask=SOBEL):
        return im.conv(mask, scale=2.0, offset=128.0, precision="integer")

    def conv2():
        conv1(SOBEL)
        return conv1(SOBEL90)

    def conv8():
        out = None
        for _ in range(8):
            out = im.conv(KIRSCH, precision="integer")
        return out

    def general_sobel():
        lib.vips_hip_vector_set_enabled(1)
        try:
            return im.sobel()
        finally:
            lib.vips_hip_vector_set_enabled(0)

    cases = [
        ("conv 3x3 integer (yardstick)", conv1),
        ("conv 3x3 integer, scale 1", lambda: im.conv(KIRSCH, precision="integer")),
        ("2 x conv 3x3 integer", conv2),
        ("sobel", im.sobel),
        ("scharr", im.scharr),
        ("prewitt", im.prewitt),
        ("sobel, general tier on uchar", general_sobel),
        ("sobel on float", imf.sobel),
        ("8 x conv 3x3 integer", conv8),
        ("compass x8 d45 max integer", lambda: im.compass(KIRSCH, times=8, angle="d45", combine="max", precision="integer")),
        ("compass x8 d45 sum integer", lambda: im.compass(KIRSCH, times=8, angle="d45", combine="sum", precision="integer")),
        ("compass x8 d45 max float", lambda: im.compass(KIRSCH, times=8, angle="d45", combine="max", precision="float")),
        ("gaussblur 1.4 integer", lambda: im.gaussblur(1.4, precision="integer")),
        ("canny 1.4 integer", lambda: im.canny(1.4, precision="integer")),
        ("gaussblur 1.4 float", lambda: im.gaussblur(1.4, precision="float")),
        ("canny 1.4 float", lambda: im.canny(1.4, precision="float")),
    ]
    say("# %d x %d x %d uchar; %d warm-up + %d timed calls a case, device events round the timed calls; one process" % (
        SIDE, SIDE, BANDS, WARM, TIMED))
    say("# %-32s %9s %8s %9s   kernels (gate: launches ms)" % ("case", "ms", "% 8TB/s", "x conv3x3"))
    yard = None
    for name, fn in cases:
        for _ in range(WARM):
            fn()
        libvips_amd.synchronize()
        e0, e1 = lib.vips_hip_event_new(), lib.vips_hip_event_new()
        assert e0 and e1
        _ffi.check(lib.vips_hip_event_record(e0))
        for _ in range(TIMED):
            fn()
        _ffi.check(lib.vips_hip_event_record(e1))
        _ffi.check(lib.vips_hip_event_synchronize(e1))
        ms = lib.vips_hip_event_elapsed_ms(e0, e1) / TIMED
        lib.vips_hip_event_free(e0)
        lib.vips_hip_event_free(e1)

        lib.vips_hip_gate_reset()
        lib.vips_hip_gate_enable(1)
        out = fn()
        libvips_amd.synchronize()
        report = libvips_amd.gate_report()
        lib.vips_hip_gate_enable(0)
        lib.vips_hip_gate_reset()
        in_bytes = src.nbytes * (4 if "float" in name and "compass" not in name else 1)
        nbytes = in_bytes + out.width * out.height * out.bands * np.dtype(libvips_amd.image.FORMAT_DTYPES[
            libvips_amd.image.FORMATS[out.format]]).itemsize
        del out
        yard = ms if yard is None else yard
        kernels = "  ".join("%s x%d %.3f" % (k, n, t) for k, (n, t) in sorted(report.items()))
        say("  %-32s %9.3f %8.1f %9.2f   %s" % (name, ms, nbytes / (ms * 1e-3) / PEAK * 100, ms / yard, kernels))
    say("PERF-OK")
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
