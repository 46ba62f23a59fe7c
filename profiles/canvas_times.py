"""What the canvas operations cost (libvips_amd/csrc/canvas.hip, ops_canvas.cpp) beside the yardsticks the library already
had, in ONE process on images resident on the device: 8192 x 8192 pels of 3 and 4 bands, uchar and ushort.

  * embed black and mirror into an 8448 x 8448 canvas (the image at 128, 128), through the streaming kernel and, for
    black, through the one-pel-a-lane kernel ($VIPS_HIP_NO_CANVAS_STREAM);
  * flatten to a white background;
  * insert of a 1024 x 1024 sub-image at (3001, 2003);
  * the yardsticks: vips_hip_memcpy_d2d of half the bytes a case reads plus writes (a copy reads and writes each of its
    bytes), cast uchar -> ushort and flip vertical -- the parent's code, not the code under test.

Every figure is device events on the library's stream round a window of calls after WARM, taken REPEATS times; the
median is reported and the spread kept.  A window holds as many calls as make it at least WINDOW_MS long (and at least
TIMED), counted from a first short window.  Every call is a Python call and a pool allocation of its result, so beside
the device time of a call the script keeps the HOST time the loop took to queue it (enqueue_ms): where that is below
the device time the queue never ran dry and the figure is the kernel's; a case where it is not is marked
"host-bound" and its figure is an upper bound of the kernel's time.  Bytes are the algorithm's: the input once plus the output once.  hbm = bytes / time over
8 TB/s; to_copy = the time of the copy of the same bytes over the case's time (1 = as fast as the copy).
Usage: canvas_times.py [output.json]   (CANVAS_PERF_SCALE=8 shrinks every side, for a rehearsal).  Needs the GPU: there
is no fallback."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCALE = int(os.environ.get("CANVAS_PERF_SCALE", "1"))
SIDE, CANVAS, SUB = 8192 // SCALE, 8448 // SCALE, 1024 // SCALE
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

    def timed(fn):
        """-> (median ms a call, [ms of every repeat], calls a window, median host ms a call)"""
        for _ in range(WARM):
            fn()
        libvips_amd.synchronize()
        first, _ = window(fn, TIMED)
        calls = max(TIMED, int(WINDOW_MS / first) + 1)
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

    rows = []

    def record(name, dtype, bands, nbytes, fn, kernel=None):
        ms, runs, calls, host = timed(fn)
        c_ms, c_runs, c_calls, c_host = copy_ms(nbytes)
        rate = nbytes / (ms * 1e-3)
        rows.append({"case": name, "format": np.dtype(dtype).name, "bands": bands, "kernel": kernel, "bytes": nbytes,
                     "ms": ms, "ms_runs": runs, "calls": calls, "enqueue_ms": host, "host_bound": host >= ms,
                     "gb_s": rate / 1e9, "hbm": rate / PEAK, "copy_ms": c_ms, "copy_ms_runs": c_runs, "copy_calls": c_calls,
                     "copy_enqueue_ms": c_host, "copy_host_bound": c_host >= c_ms, "to_copy": c_ms / ms})
        print("%-26s %-6s x%d  %8.3f ms (%5d calls, queued in %.3f ms each%s)  %8.1f GB/s  %5.1f %% of 8 TB/s   copy %8.3f ms "
              "(queued in %.3f%s)   to_copy %.2f" %
              (name, np.dtype(dtype).name, bands, ms, calls, host, ", HOST-BOUND" if host >= ms else "", rate / 1e9,
               100 * rate / PEAK, c_ms, c_host, ", HOST-BOUND" if c_host >= c_ms else "", c_ms / ms), flush=True)

    rng = np.random.default_rng(7)
    for dtype in (np.uint8, np.uint16):
        for bands in (3, 4):
            es = np.dtype(dtype).itemsize
            src = rng.integers(0, 256, (SIDE, SIDE, bands), dtype=np.uint8).astype(dtype)
            im = Image.new_from_array(src, "srgb" if dtype == np.uint8 else "rgb16")
            sub = Image.new_from_array(src[:SUB, :SUB], "srgb" if dtype == np.uint8 else "rgb16")
            in_b, canvas_b = SIDE * SIDE * bands * es, CANVAS * CANVAS * bands * es
            pad = (CANVAS - SIDE) // 2
            record("embed black", dtype, bands, in_b + canvas_b, lambda: im.embed(pad, pad, CANVAS, CANVAS), "canvas_stream")
            record("embed mirror", dtype, bands, in_b + canvas_b, lambda: im.embed(pad, pad, CANVAS, CANVAS, extend="mirror"),
                   "canvas_stream")
            os.environ["VIPS_HIP_NO_CANVAS_STREAM"] = "1"
            try:
                record("embed black (general)", dtype, bands, in_b + canvas_b, lambda: im.embed(pad, pad, CANVAS, CANVAS),
                       "canvas_general")
            finally:
                del os.environ["VIPS_HIP_NO_CANVAS_STREAM"]
            white = 255 if dtype == np.uint8 else 65535
            record("flatten white", dtype, bands, in_b + in_b // bands * (bands - 1), lambda: im.flatten(background=white),
                   "flatten_u8" if dtype == np.uint8 else "flatten_any")
            record("insert %d^2" % SUB, dtype, bands, 2 * in_b, lambda: im.insert(sub, 3001 // SCALE, 2003 // SCALE), "canvas_stream")
            record("flip vertical", dtype, bands, 2 * in_b, lambda: im.flipver(), "flip_stream")
            if dtype == np.uint8:
                record("cast uchar -> ushort", dtype, bands, 3 * in_b, lambda: im.cast("ushort"), "cast")
            del im, sub
            lib.vips_hip_pool_trim()
    lib.vips_hip_event_free(e0)
    lib.vips_hip_event_free(e1)
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "canvas_times.json")
    with open(out, "w") as f:
        json.dump({"side": SIDE, "canvas": CANVAS, "sub": SUB, "warm": WARM, "timed": TIMED, "window_ms": WINDOW_MS, "repeats": REPEATS,
                   "peak_bytes_s": PEAK, "rows": rows}, f, indent=1)
        f.write("\n")
    print("PERF-OK " + out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
