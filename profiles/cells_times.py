"""What the sheet operations cost (libvips_amd/csrc/cells.hip, ops_cells.cpp) beside the yardsticks the library already had,
in ONE process on images resident on the device.

  * arrayjoin of 256 RGB 256 x 256 uchar images across 16, the same with a shim of 2 (a sheet whose rows are no whole
    dwords: the one-pel-a-lane kernel), and the same sheet made the old way, by 255 join calls (rows of 16, then the
    rows under one another): the figure the feature replaces;
  * arrayjoin of 1024 RGBA 64 x 64 images across 32;
  * replicate 4 x 4 of a 2048 x 2048 x 3 image, beside embed(extend="repeat") to the same canvas on the canvas kernel;
  * grid of a 256 x 65536 x 3 strip to 16 x 16 tiles; wrap of 8192 x 8192 x 3;
  * in the same run, embed black (8192^2 -> 8448^2) and insert of a 1024^2 sub-image for the same pel sizes: the parent's
    code, not the code under test, which DESIGN.md 3.5h records at 0.81-0.96 of a copy;
  * the yardstick of every case: vips_hip_memcpy_d2d of half the bytes the case reads plus writes (a copy reads and
    writes each of its bytes).

Every figure is device events on the library's stream round a window of calls after WARM, taken REPEATS times; the
median is reported and the spread kept.  A window holds as many calls as make it at least WINDOW_MS long (and at least
`least` calls), counted from a first short window.  Every call is a Python call and a pool allocation of its result --
and, for arrayjoin, the upload of its table of descriptors, which waits for the stream -- so beside the device time of
a call the script keeps the HOST time the loop took to queue it (enqueue_ms): where that is below the device time the
queue never ran dry and the figure is the kernel's; a case where it is not is marked "host-bound" and its figure is an
upper bound of the kernel's time.  Bytes are the algorithm's: the input once plus the output once.  hbm = bytes / time
over 8 TB/s; to_copy = the time of the copy of the same bytes over the case's time (1 = as fast as the copy).
Usage: cells_times.py [output.json]   (CELLS_PERF_SCALE=8 shrinks every side, for a rehearsal).  Needs the GPU: there
is no fallback."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCALE = int(os.environ.get("CELLS_PERF_SCALE", "1"))
THUMB, SMALL, TILE, SIDE, CANVAS, SUB = 256 // SCALE, 64 // SCALE, 2048 // SCALE, 8192 // SCALE, 8448 // SCALE, 1024 // SCALE
WARM, TIMED, REPEATS = 5, 200, 3
WINDOW_MS = 300.0
PEAK = 8e12


def main():
    import libvips_amd
    from libvips_amd import Image, _ffi

    lib = _ffi.lib
    libvips_amd.init(0)
    e0, e1 = lib.vips_hip_event_new(), lib.vips_hip_event_new()
    assert e0 and e1

    def window(fn, calls):
        """-> (device ms a call, host ms a call spent queueing)"""
        _ffi.check(lib.vips_hip_event_record(e0))
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        host = (time.perf_counter() - t0) * 1e3 / calls
        _ffi.check(lib.vips_hip_event_record(e1))
        _ffi.check(lib.vips_hip_event_synchronize(e1))
        return lib.vips_hip_event_elapsed_ms(e0, e1) / calls, host

    def timed(fn, least=TIMED):
        """-> (median ms a call, [ms of every repeat], calls a window, median host ms a call)"""
        for _ in range(WARM):
            fn()
        libvips_amd.synchronize()
        first, _ = window(fn, least)
        calls = max(least, int(WINDOW_MS / first) + 1)
        runs = [window(fn, calls) for _ in range(REPEATS)]
        return float(np.median([r[0] for r in runs])), [r[0] for r in runs], calls, float(np.median([r[1] for r in runs]))

    def copy_ms(nbytes):
        half = nbytes // 2
        a, b = lib.vips_hip_malloc(half), lib.vips_hip_malloc(half)
        assert a and b
        try:
            return timed(lambda: _ffi.check(lib.vips_hip_memcpy_d2d(b, a, half)))
        finally:
            lib.vips_hip_free(a)
            lib.vips_hip_free(b)

    def kernels_of(fn):
        """{gate name: launches} of one call"""
        lib.vips_hip_gate_reset()
        lib.vips_hip_gate_enable(1)
        try:
            fn()
            libvips_amd.synchronize()
            return {k: n for k, (n, _) in libvips_amd.gate_report().items()}
        finally:
            lib.vips_hip_gate_enable(0)
            lib.vips_hip_gate_reset()

    rows = []

    def record(name, shape, nbytes, fn, least=TIMED):
        kernels = kernels_of(fn)
        ms, runs, calls, host = timed(fn, least)
        c_ms, c_runs, c_calls, c_host = copy_ms(nbytes)
        rate = nbytes / (ms * 1e-3)
        rows.append({"case": name, "shape": shape, "kernels": kernels, "bytes": nbytes, "ms": ms, "ms_runs": runs, "calls": calls,
                     "enqueue_ms": host, "host_bound": host >= ms, "gb_s": rate / 1e9, "hbm": rate / PEAK, "copy_ms": c_ms,
                     "copy_ms_runs": c_runs, "copy_calls": c_calls, "copy_enqueue_ms": c_host, "copy_host_bound": c_host >= c_ms,
                     "to_copy": c_ms / ms})
        print("%-34s %-22s %8.3f ms (%5d calls, queued in %.3f ms each%s)  %8.1f GB/s  %5.1f %% of 8 TB/s   copy %8.3f ms "
              "(queued in %.3f%s)   to_copy %.2f   %s" %
              (name, shape, ms, calls, host, ", HOST-BOUND" if host >= ms else "", rate / 1e9, 100 * rate / PEAK, c_ms, c_host,
               ", HOST-BOUND" if c_host >= c_ms else "", c_ms / ms, kernels), flush=True)

    rng = np.random.default_rng(7)

    def images(n, side, bands):
        return [Image.new_from_array(rng.integers(0, 256, (side, side, bands), dtype=np.uint8), "srgb") for _ in range(n)]

    # ---- the contact sheet
    thumbs = images(256, THUMB, 3)
    in_b = 256 * THUMB * THUMB * 3
    record("arrayjoin 256 across 16", "%d^2 x 3 uchar" % THUMB, 2 * in_b, lambda: Image.arrayjoin(thumbs, across=16))
    shim_b = (16 * THUMB + 30) ** 2 * 3
    record("arrayjoin 256 across 16, shim 2", "%d^2 x 3 uchar" % THUMB, in_b + shim_b,
           lambda: Image.arrayjoin(thumbs, across=16, shim=2, background=255))

    def by_joins():
        strips = []
        for r in range(16):
            row = thumbs[16 * r]
            for im in thumbs[16 * r + 1:16 * r + 16]:
                row = row.join(im, "horizontal")
            strips.append(row)
        sheet = strips[0]
        for row in strips[1:]:
            sheet = sheet.join(row, "vertical")
        return sheet

    record("the same sheet by 255 joins", "%d^2 x 3 uchar" % THUMB, 2 * in_b, by_joins, least=10)
    del thumbs
    small = images(1024, SMALL, 4)
    in_b = 1024 * SMALL * SMALL * 4
    record("arrayjoin 1024 across 32", "%d^2 x 4 uchar" % SMALL, 2 * in_b, lambda: Image.arrayjoin(small, across=32))
    del small
    lib.vips_hip_pool_trim()

    # ---- one image
    tile = images(1, TILE, 3)[0]
    in_b, out_b = TILE * TILE * 3, 16 * TILE * TILE * 3
    record("replicate 4 x 4", "%d^2 x 3 uchar" % TILE, in_b + out_b, lambda: tile.replicate(4, 4))
    record("embed repeat to the same canvas", "%d^2 x 3 uchar" % TILE, in_b + out_b,
           lambda: tile.embed(0, 0, 4 * TILE, 4 * TILE, extend="repeat"))
    del tile
    strip = Image.new_from_array(rng.integers(0, 256, (256 * THUMB, THUMB, 3), dtype=np.uint8), "srgb")
    in_b = 256 * THUMB * THUMB * 3
    record("grid 16 x 16", "%d x %d x 3 uchar" % (THUMB, 256 * THUMB), 2 * in_b, lambda: strip.grid(THUMB, 16, 16))
    del strip
    lib.vips_hip_pool_trim()
    for bands in (3, 4):
        im = images(1, SIDE, bands)[0]
        sub = images(1, SUB, bands)[0]
        in_b, canvas_b = SIDE * SIDE * bands, CANVAS * CANVAS * bands
        pad = (CANVAS - SIDE) // 2
        shape = "%d^2 x %d uchar" % (SIDE, bands)
        record("wrap", shape, 2 * in_b, lambda: im.wrap())
        record("replicate 1 x 1 (a copy)", shape, 2 * in_b, lambda: im.replicate(1, 1))
        record("embed black -> %d^2" % CANVAS, shape, in_b + canvas_b, lambda: im.embed(pad, pad, CANVAS, CANVAS))
        record("insert %d^2" % SUB, shape, 2 * in_b, lambda: im.insert(sub, 3001 // SCALE, 2003 // SCALE))
        del im, sub
        lib.vips_hip_pool_trim()
    lib.vips_hip_event_free(e0)
    lib.vips_hip_event_free(e1)
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "cells_times.json")
    with open(out, "w") as f:
        json.dump({"thumb": THUMB, "small": SMALL, "tile": TILE, "side": SIDE, "canvas": CANVAS, "sub": SUB, "warm": WARM,
                   "timed": TIMED, "window_ms": WINDOW_MS, "repeats": REPEATS, "peak_bytes_s": PEAK, "rows": rows}, f, indent=1)
        f.write("\n")
    print("PERF-OK " + out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
