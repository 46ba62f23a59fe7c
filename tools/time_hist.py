"""What the histogram operations cost (libvips_amd/csrc/hist.hip, hist_local.hip, ops_histogram.cpp), on an 8192 x 8192 x
3 uchar image resident on the device:

  * hist_equal (the histogram kernel, 1 KB a band to the host and back, maplut_u8) and maplut through a 256-entry uchar
    table;
  * stdif 11 x 11;
  * hist_local 15 x 15 and 63 x 63 with max_slope 0 and 3 (CLAHE).

Every case is a process of its own under `timeout` (the parent stops at the first one that fails) and reports: ms a
call (device events on the library's stream round TIMED calls after WARM), the algorithmic bytes (input + output, once
each) over that time in GB/s and as a fraction of 8 TB/s, the kernels that ran (gate report: launches, ms), and the
reference's time for the same call on the host cores (Ref.time_chain: graph build + full evaluation into memory; for
maplut, whose table is an image argument, the wall time of the shim's call).
Usage: time_hist.py [output file]   (HIST_PERF_SCALE=8 shrinks every side, for a rehearsal; HIST_PERF_REF=0 leaves the
reference out; --case N runs one case alone, for a profiler)"""
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCALE = int(os.environ.get("HIST_PERF_SCALE", "1"))
WITH_REF = os.environ.get("HIST_PERF_REF", "1") != "0"
SIDE = 8192 // SCALE
BANDS = 3
WARM, TIMED = 2, 6
PEAK = 8e12
STEP_SECONDS = 400

# name -> (kind, arguments)
CASES = [
    ("hist_equal", "hist_equal", ()),
    ("maplut 256 x uchar", "maplut", ()),
    ("stdif 11x11", "stdif", (11, 11)),
    ("hist_local 15x15", "hist_local", (15, 15, 0)),
    ("hist_local 15x15 max_slope 3", "hist_local", (15, 15, 3)),
    ("hist_local 63x63", "hist_local", (63, 63, 0)),
    ("hist_local 63x63 max_slope 3", "hist_local", (63, 63, 3)),
]


def one_case(number):
    import libvips_amd
    from libvips_amd import Image, _ffi
    from tests import helpers
    from tests.helpers import Ref

    lib = _ffi.lib
    libvips_amd.init(0)
    name, kind, args = CASES[number]
    src = helpers.lcg_image(SIDE, SIDE, BANDS, np.uint8, 5)
    im = Image.new_from_array(src)
    table = (255 - np.arange(256)).astype(np.uint8).reshape(1, 256, 1)
    lut = Image.new_from_array(table, "histogram")
    if kind == "hist_equal":
        fn = lambda: im.hist_equal()  # noqa: E731
    elif kind == "maplut":
        fn = lambda: im.maplut(lut)  # noqa: E731
    elif kind == "stdif":
        fn = lambda: im.stdif(*args)  # noqa: E731
    else:
        fn = lambda: im.hist_local(*args)  # noqa: E731

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
        if kind == "hist_equal":
            ref_ms = Ref.time_chain("hist_equal", src, repeats=1) * 1e3
        elif kind == "maplut":
            with tempfile.TemporaryDirectory() as tmp:
                path = os.path.join(tmp, "lut.v")
                helpers.write_v(path, table, interpretation=10)
                t0 = time.perf_counter()
                Ref.run("maplut", src, "lut=" + path)
                ref_ms = (time.perf_counter() - t0) * 1e3
        elif kind == "stdif":
            ref_ms = Ref.time_chain("stdif:width=%d,height=%d" % args, src, repeats=1) * 1e3
        else:
            ref_ms = Ref.time_chain("hist_local:width=%d,height=%d,max-slope=%d" % args, src, repeats=1) * 1e3
    kernels = "  ".join("%s x%d %.3f" % (k, n, t) for k, (n, t) in sorted(report.items()))
    print("RESULT\t%s\t%.4f\t%d\t%.1f\t%s" % (name, ms, nbytes, ref_ms, kernels), flush=True)


def main():
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say("# %d x %d x %d uchar, input resident; %d warm-up + %d timed calls a case, device events round the timed calls; a "
        "process a case" % (SIDE, SIDE, BANDS, WARM, TIMED))
    say("# the device's clocks as found: nothing sets or reads them; the reference on the same machine's host cores")
    say("# %-30s %9s %9s %8s %11s %8s   kernels (gate: launches ms)" % ("case", "ms", "GB/s", "% 8TB/s", "ref ms", "ref / us"))
    for number, case in enumerate(CASES):
        proc = subprocess.run(["timeout", "-k", "10", str(STEP_SECONDS), sys.executable, os.path.abspath(__file__), "--case", str(number)],
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        result = [l for l in proc.stdout.splitlines() if l.startswith("RESULT\t")]
        if proc.returncode != 0 or not result:
            say("FAILED %s (exit %d): %s" % (case[0], proc.returncode, proc.stdout[-2000:]))
            return 1
        _, name, ms, nbytes, ref_ms, kernels = result[0].split("\t")
        ms, nbytes, ref_ms = float(ms), int(nbytes), float(ref_ms)
        rate = nbytes / (ms * 1e-3)
        say("  %-30s %9.3f %9.1f %8.2f %11.1f %8.0f   %s" % (name, ms, rate / 1e9, rate / PEAK * 100, ref_ms, ref_ms / ms, kernels))
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
