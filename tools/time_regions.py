"""What labelregions and countlines cost (libvips_amd/csrc/regions.hip, ops_regions.cpp), on an 8192 x 8192 one-band
uchar image resident on the device, for three contents:

  * noise      two-value noise: the worst case, most pels are seam or root work;
  * blobs      noise blurred (a 33-pel box, twice) and thresholded at its median: a few thousand blobs, the realistic case;
  * constant   one region.

Every case is a process of its own under `timeout` (the parent stops at the first one that fails) and reports: ms a
call (device events on the library's stream round TIMED calls after WARM) for labelregions with `segments` (its one
download included) and for countlines both ways; for every pass of labelregions the time from its gate and, beside it,
the bytes the pass must read and write as counted from the code (what depends on the content -- the walks to a root, the
seam unions, the roots' own writes -- is left out: the floor, not the traffic), and that floor over the time in GB/s;
the regions found; the reference's time for the same call on the same machine's host (the wall time of `vips
labelregions in.v mask.v` / `vips countlines in.v <direction>`, which maps the file and, for labelregions, writes the
mask; vips_labelregions is single-threaded).
Usage: time_regions.py [output file]   (REGIONS_PERF_SCALE=8 shrinks every side, for a rehearsal; REGIONS_PERF_REF=0
leaves the reference out; --case N runs one case alone, for a profiler)"""
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCALE = int(os.environ.get("REGIONS_PERF_SCALE", "1"))
WITH_REF = os.environ.get("REGIONS_PERF_REF", "1") != "0"
SIDE = 8192 // SCALE
WARM, TIMED = 2, 6
PEAK = 8e12
STEP_SECONDS = 400
CASES = ["noise", "blobs", "constant"]
PASSES = ("label_tiles", "label_seams", "label_roots", "label_scan", "label_serials", "label_number")


def content(name):
    from tests import helpers

    if name == "constant":
        return np.full((SIDE, SIDE, 1), 255, np.uint8)
    noise = helpers.lcg_image(SIDE, SIDE, 1, np.uint8, 5)
    if name == "noise":
        return (noise & 1) * np.uint8(255)
    box = max(3, 33 // SCALE) | 1
    v = noise[:, :, 0].astype(np.float32)
    for _ in range(2):
        for axis in (0, 1):
            c = np.cumsum(np.pad(v, [(box // 2 + 1, box // 2) if a == axis else (0, 0) for a in (0, 1)], mode="wrap"), axis=axis,
                          dtype=np.float64)
            v = (np.take(c, np.arange(box, box + SIDE), axis=axis) - np.take(c, np.arange(0, SIDE), axis=axis)).astype(np.float32) / box
    return ((v >= np.median(v)) * np.uint8(255)).astype(np.uint8)[:, :, None]


def floors(n, step):
    """pass -> (bytes read, bytes written) that do not depend on the content, n one-byte pels: the input once; the int
    parent plane written by label_tiles, read by label_roots; the int output plane written by label_roots, read by
    label_serials and label_number, written by label_number; label_number's gather from the parent plane; the seams' 5 /
    64 of a byte a pel written and read; the chunk counts."""
    tw, th, chunk = step
    seams = n // tw + n // th
    counts = 4 * (n // chunk)
    return {
        "label_tiles": (n, 4 * n + seams),
        "label_seams": (seams, 0),
        "label_roots": (4 * n, 4 * n + counts),
        "label_scan": (counts, counts),
        "label_serials": (4 * n + counts, 0),
        "label_number": (8 * n, 4 * n),
    }


def timed(lib, ffi, fn):
    import libvips_amd

    for _ in range(WARM):
        fn()
    libvips_amd.synchronize()
    e0, e1 = lib.vips_hip_event_new(), lib.vips_hip_event_new()
    assert e0 and e1
    ffi.check(lib.vips_hip_event_record(e0))
    for _ in range(TIMED):
        fn()
    ffi.check(lib.vips_hip_event_record(e1))
    ffi.check(lib.vips_hip_event_synchronize(e1))
    ms = lib.vips_hip_event_elapsed_ms(e0, e1) / TIMED
    lib.vips_hip_event_free(e0)
    lib.vips_hip_event_free(e1)
    return ms


def one_case(number):
    import libvips_amd
    from libvips_amd import Image, _ffi
    from tests import helpers

    lib = _ffi.lib
    libvips_amd.init(0)
    name = CASES[number]
    src = content(name)
    im = Image.new_from_array(src)
    label_ms = timed(lib, _ffi, lambda: im.labelregions(with_options=True))
    lines_ms = [timed(lib, _ffi, lambda d=d: im.countlines(d)) for d in ("horizontal", "vertical")]

    lib.vips_hip_gate_reset()
    lib.vips_hip_gate_enable(1)
    _, opts = im.labelregions(with_options=True)
    lines = [im.countlines(d) for d in ("horizontal", "vertical")]
    libvips_amd.synchronize()
    report = libvips_amd.gate_report()
    lib.vips_hip_gate_enable(0)
    lib.vips_hip_gate_reset()

    ref = [float("nan")] * 3
    if WITH_REF and helpers.have_ref():
        vips = os.path.join(ROOT, "oracle", "_ref", "bin", "vips")
        with tempfile.TemporaryDirectory() as tmp:
            path, out = os.path.join(tmp, "in.v"), os.path.join(tmp, "mask.v")
            helpers.write_v(path, src, 1)
            for i, args in enumerate((["labelregions", path, out], ["countlines", path, "horizontal"], ["countlines", path, "vertical"])):
                t0 = time.perf_counter()
                subprocess.run([vips] + args, env=helpers.ref_cli_env(), check=True, stdout=subprocess.DEVNULL)
                ref[i] = (time.perf_counter() - t0) * 1e3
    step = (lib.vips_hip_labelregions_step(0), lib.vips_hip_labelregions_step(1), 1024)
    fl = floors(SIDE * SIDE, step)
    passes = ";".join("%s,%.4f,%d,%d" % (k, report.get(k, (0, 0.0))[1], fl[k][0], fl[k][1]) for k in PASSES)
    print("RESULT\t%s\t%.4f\t%.4f\t%.4f\t%d\t%r\t%r\t%.1f\t%.1f\t%.1f\t%.4f\t%s" % (
        name, label_ms, lines_ms[0], lines_ms[1], opts["segments"] - 1, lines[0], lines[1], ref[0], ref[1], ref[2],
        report.get("countlines", (0, 0.0))[1] / 2, passes), flush=True)


def main():
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    n = SIDE * SIDE
    say("# %d x %d x 1 uchar, input resident; %d warm-up + %d timed calls a case, device events round the timed calls; a process a "
        "case" % (SIDE, SIDE, WARM, TIMED))
    say("# the device's clocks as found: nothing sets or reads them; the reference on the same machine's host (command line, one thread "
        "for labelregions)")
    say("# floor: the bytes a pass reads + writes whatever the content, counted from the code; GB/s: that floor over the pass's time")
    for number, case in enumerate(CASES):
        proc = subprocess.run(["timeout", "-k", "10", str(STEP_SECONDS), sys.executable, os.path.abspath(__file__), "--case", str(number)],
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        result = [l for l in proc.stdout.splitlines() if l.startswith("RESULT\t")]
        if proc.returncode != 0 or not result:
            say("FAILED %s (exit %d): %s" % (case, proc.returncode, proc.stdout[-2000:]))
            return 1
        f = result[0].split("\t")
        name, label_ms, h_ms, v_ms, regions = f[1], float(f[2]), float(f[3]), float(f[4]), int(f[5])
        ref = [float(x) for x in f[8:11]]
        say("%s: %d regions, countlines %s / %s" % (name, regions, f[6], f[7]))
        total = n + 4 * n
        say("  %-22s %9.3f ms   %7.1f GB/s of input + mask   reference %9.1f ms (%.0f x)" % (
            "labelregions", label_ms, total / (label_ms * 1e-3) / 1e9, ref[0], ref[0] / label_ms))
        floor_sum = 0
        for item in f[12].split(";"):
            k, ms, rd, wr = item.split(",")
            ms, rd, wr = float(ms), int(rd), int(wr)
            floor_sum += rd + wr
            rate = (rd + wr) / (ms * 1e-3) / 1e9 if ms > 0 else float("nan")
            say("    %-20s %9.3f ms   read %11d  written %11d   %7.1f GB/s  %5.2f %% of 8 TB/s" % (k, ms, rd, wr, rate, rate * 1e9 / PEAK * 100))
        say("    %-20s floor of all passes %d bytes = %.2f per pel" % ("", floor_sum, floor_sum / n))
        for d, ms, r in (("horizontal", h_ms, ref[1]), ("vertical", v_ms, ref[2])):
            say("  %-22s %9.3f ms   %7.1f GB/s of input   reference %9.1f ms (%.0f x)" % (
                "countlines " + d, ms, n / (ms * 1e-3) / 1e9, r, r / ms))
        say("    %-20s %9.3f ms   (gate, mean of the two directions)" % ("countlines", float(f[11])))
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
