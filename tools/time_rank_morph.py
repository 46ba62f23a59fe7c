"""What the rank and morphology filters cost (libvips_amd/csrc/rank.hip, morph.hip), on an 8192 x 8192 x 3 uchar image
unless the case says otherwise:

  * the yardstick: the integer 3 x 3 convolution of the same image (it stages the same halo tile);
  * median 3 x 3 and 5 x 5, rank 11 x 11 index 60, rank 15 x 15 min and max, median 3 x 3 on ushort and on float;
  * erode and dilate with a 3 x 3 cross, a full 3 x 3, a full 5 x 5 and a 9 x 9 disc.

Every case is a process of its own under `timeout` (the parent stops at the first one that fails) and reports: ms a
call (device events on the library's stream round TIMED calls after WARM), the algorithmic bytes (input + output, once
each) over that time as a fraction of 8 TB/s, the ratio to the yardstick measured in the same run, the kernels that
ran (gate report), and the reference's time for the same call on the host cores (Ref.time_chain: graph build + full
evaluation into memory, best of 2; for morph, whose mask is an image argument, the wall time of the shim's call).
Usage: time_rank_morph.py [output file]   (RANK_PERF_SCALE=8 shrinks every side, for a rehearsal;
RANK_PERF_REF=0 leaves the reference out)"""
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCALE = int(os.environ.get("RANK_PERF_SCALE", "1"))
WITH_REF = os.environ.get("RANK_PERF_REF", "1") != "0"
SIDE = 8192 // SCALE
BANDS = 3
WARM, TIMED = 3, 10
PEAK = 8e12
STEP_SECONDS = 240


def disc(side):
    y, x = np.mgrid[0:side, 0:side]
    r = (side - 1) / 2.0
    return np.where((x - r) ** 2 + (y - r) ** 2 <= r * r + 0.5, 255.0, 128.0)


CROSS3 = np.array([[128, 255, 128], [255, 255, 255], [128, 255, 128]], float)
# name -> (kind, dtype, arguments)
CASES = [
    ("conv 3x3 integer (yardstick)", "conv", np.uint8, None),
    ("median 3x3", "rank", np.uint8, (3, 3, 4)),
    ("median 5x5", "rank", np.uint8, (5, 5, 12)),
    ("rank 11x11 index 60", "rank", np.uint8, (11, 11, 60)),
    ("rank 15x15 min", "rank", np.uint8, (15, 15, 0)),
    ("rank 15x15 max", "rank", np.uint8, (15, 15, 224)),
    ("median 3x3 ushort", "rank", np.uint16, (3, 3, 4)),
    ("median 3x3 float", "rank", np.float32, (3, 3, 4)),
    ("erode 3x3 cross", "morph", np.uint8, (CROSS3, "erode")),
    ("dilate 3x3 cross", "morph", np.uint8, (CROSS3, "dilate")),
    ("erode 3x3 full", "morph", np.uint8, (np.full((3, 3), 255.0), "erode")),
    ("dilate 3x3 full", "morph", np.uint8, (np.full((3, 3), 255.0), "dilate")),
    ("erode 5x5 full", "morph", np.uint8, (np.full((5, 5), 255.0), "erode")),
    ("dilate 5x5 full", "morph", np.uint8, (np.full((5, 5), 255.0), "dilate")),
    ("erode 9x9 disc", "morph", np.uint8, (disc(9), "erode")),
    ("dilate 9x9 disc", "morph", np.uint8, (disc(9), "dilate")),
]


def one_case(number):
    import libvips_amd
    from libvips_amd import Image, _ffi
    from tests import helpers
    from tests.helpers import Ref

    lib = _ffi.lib
    libvips_amd.init(0)
    name, kind, dtype, args = CASES[number]
    src = helpers.lcg_image(SIDE, SIDE, BANDS, dtype, 5)
    im = Image.new_from_array(src)
    if kind == "conv":
        mask = np.array([[1, 2, 1], [2, 4, 2], [1, 2, 1]], float)
        fn = lambda: im.conv(mask, scale=16.0, precision="integer")  # noqa: E731
    elif kind == "rank":
        fn = lambda: im.rank(*args)  # noqa: E731
    else:
        fn = lambda: im.morph(*args)  # noqa: E731

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
    nbytes = src.nbytes + out.numpy().nbytes

    ref_ms = float("nan")
    if WITH_REF and helpers.have_ref():
        if kind == "rank":
            ref_ms = Ref.time_chain("rank:width=%d,height=%d,index=%d" % args, src, repeats=2) * 1e3
        elif kind == "conv":
            t0 = time.perf_counter()
            Ref.run_mask("conv", src, mask, 16.0, 0.0, args="precision=integer")
            ref_ms = (time.perf_counter() - t0) * 1e3
        else:
            t0 = time.perf_counter()
            Ref.run_mask("morph", src, args[0], args="morph=" + args[1])
            ref_ms = (time.perf_counter() - t0) * 1e3
    kernels = "  ".join("%s x%d %.3f" % (k, n, t) for k, (n, t) in sorted(report.items()))
    print("RESULT\t%s\t%.4f\t%d\t%.1f\t%s" % (name, ms, nbytes, ref_ms, kernels), flush=True)


def main():
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say("# %d x %d x %d; %d warm-up + %d timed calls a case, device events round the timed calls; a process a case" % (
        SIDE, SIDE, BANDS, WARM, TIMED))
    say("# %-30s %9s %8s %9s %11s %8s   kernels (gate: launches ms)" % ("case", "ms", "% 8TB/s", "x conv3x3", "ref ms", "ref / us"))
    yard = None
    for number, case in enumerate(CASES):
        proc = subprocess.run(["timeout", "-k", "10", str(STEP_SECONDS), sys.executable, os.path.abspath(__file__), "--case", str(number)],
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        result = [l for l in proc.stdout.splitlines() if l.startswith("RESULT\t")]
        if proc.returncode != 0 or not result:
            say("FAILED %s (exit %d): %s" % (case[0], proc.returncode, proc.stdout[-2000:]))
            return 1
        _, name, ms, nbytes, ref_ms, kernels = result[0].split("\t")
        ms, nbytes, ref_ms = float(ms), int(nbytes), float(ref_ms)
        yard = ms if yard is None else yard
        say("  %-30s %9.3f %8.1f %9.2f %11.1f %8.0f   %s" % (name, ms, nbytes / (ms * 1e-3) / PEAK * 100, ms / yard, ref_ms,
                                                           ref_ms / ms, kernels))
    say("PERF-OK")
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--case":
        one_case(int(sys.argv[2]))
    else:
        sys.exit(main())
