"""What the arithmetic operations cost (libvips_amd/csrc/arith.hip, ops_arith.cpp) beside the yardsticks the library already
had, in ONE process on images resident on the device: 8192 x 8192 pels, 3 bands of uchar and 4 bands of float.

  * linear in its three output forms (one constant -> float, a band vector -> float, one constant -> uchar), invert, add
    and divide, each against vips_hip_memcpy_d2d of half the bytes the case reads plus writes (a copy reads and writes
    each of its bytes);
  * stats, against hist_find of the same image where hist_find takes it (uchar), and against the copy of the bytes it
    reads.

Every figure is device events on the library's stream round a window of calls after WARM, taken REPEATS times; the
median is reported and the spread kept.  A window holds as many calls as make it at least WINDOW_MS long (and at least
TIMED), counted from a first short window.  Every call is a Python call and a pool allocation of its result (stats and
hist_find also wait for their result), so beside the device time of a call the script keeps the HOST time the loop took
to queue it (enqueue_ms): where that is below the device time the queue never ran dry and the figure is the kernel's; a
case where it is not is marked "host-bound" and its figure is an upper bound of the kernel's time.  Bytes are the
algorithm's: every input once plus the output once.  hbm = bytes / time over 8 TB/s; to_copy = the time of the copy of
the same bytes over the case's time (1 = as fast as the copy).
Usage: arith_times.py [output.json]   (ARITH_PERF_SCALE=8 shrinks every side, for a rehearsal).  Needs the GPU: there is
no fallback."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCALE = int(os.environ.get("ARITH_PERF_SCALE", "1"))
SIDE = 8192 // SCALE
WARM, TIMED, REPEATS = 3, 20, 3
WINDOW_MS = 200.0
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
        calls = max(TIMED, int(WINDOW_MS / max(first, 1e-3)) + 1)
        runs = [window(fn, calls) for _ in range(REPEATS)]
        # (a runtime whose events do not tick -- the CPU suite's mock -- must not divide by zero)
        return max(float(np.median([r[0] for r in runs])), 1e-6), [r[0] for r in runs], calls, float(np.median([r[1] for r in runs]))

    copies = {}

    def copy_ms(nbytes):
        if nbytes not in copies:
            half = nbytes // 2
            a, b = lib.vips_hip_malloc(half), lib.vips_hip_malloc(half)
            assert a and b
            try:
                copies[nbytes] = timed(lambda: _ffi.check(lib.vips_hip_memcpy_d2d(b, a, half)))
            finally:
                lib.vips_hip_free(a)
                lib.vips_hip_free(b)
        return copies[nbytes]

    rows = []

    def record(name, dtype, bands, nbytes, fn, kernel, against=None):
        ms, runs, calls, host = timed(fn)
        c_ms, c_runs, c_calls, c_host = copy_ms(nbytes)
        rate = nbytes / (ms * 1e-3)
        row = {"case": name, "format": np.dtype(dtype).name, "bands": bands, "kernel": kernel, "bytes": nbytes, "ms": ms,
               "ms_runs": runs, "calls": calls, "enqueue_ms": host, "host_bound": host >= ms, "gb_s": rate / 1e9,
               "hbm": rate / PEAK, "copy_ms": c_ms, "copy_ms_runs": c_runs, "copy_calls": c_calls, "copy_enqueue_ms": c_host,
               "copy_host_bound": c_host >= c_ms, "to_copy": c_ms / ms}
        if against:
            row["against"], row["against_ms"] = against
            row["to_against"] = against[1] / ms
        rows.append(row)
        print("%-26s %-7s x%d  %8.3f ms (%5d calls, queued in %.3f ms each%s)  %8.1f GB/s  %5.1f %% of 8 TB/s   copy %8.3f ms   "
              "to_copy %.2f%s" % (name, np.dtype(dtype).name, bands, ms, calls, host, ", HOST-BOUND" if host >= ms else "",
                                  rate / 1e9, 100 * rate / PEAK, c_ms, c_ms / ms,
                                  "   %s %.3f ms, ratio %.2f" % (against[0], against[1], against[1] / ms) if against else ""), flush=True)
        return ms

    rng = np.random.default_rng(7)
    for dtype, bands in ((np.uint8, 3), (np.float32, 4)):
        es = np.dtype(dtype).itemsize
        n = SIDE * SIDE * bands
        src = rng.integers(0, 256, (SIDE, SIDE, bands), dtype=np.uint8).astype(dtype)
        other = np.ascontiguousarray(src[::-1])
        im, im2 = Image.new_from_array(src, "srgb"), Image.new_from_array(other, "srgb")
        del src, other
        out_es = 8 if dtype == np.float64 else 4
        in_b = n * es
        vector = [1.1, 1.1, -2.5, 0.3][:bands]
        record("linear -> float", dtype, bands, in_b + n * out_es, lambda: im.linear(1.1, -20.3), "arith_stream")
        record("linear vector -> float", dtype, bands, in_b + n * out_es, lambda: im.linear(vector, -20.3), "arith_stream")
        record("linear -> uchar", dtype, bands, in_b + n, lambda: im.linear(1.1, -20.3, uchar=True), "arith_stream")
        record("invert", dtype, bands, 2 * in_b, lambda: im.invert(), "arith_stream")
        sum_es = 2 if dtype == np.uint8 else 4
        record("add", dtype, bands, 2 * in_b + n * sum_es, lambda: im.add(im2), "arith_stream")
        record("divide", dtype, bands, 2 * in_b + n * 4, lambda: im.divide(im2), "arith_stream")
        os.environ["VIPS_HIP_NO_ARITH_STREAM"] = "1"
        try:
            record("invert (general)", dtype, bands, 2 * in_b, lambda: im.invert(), "arith_general")
        finally:
            del os.environ["VIPS_HIP_NO_ARITH_STREAM"]
        against = None
        if dtype == np.uint8:
            against = ("hist_find", record("hist_find", dtype, bands, 2 * in_b, lambda: im.hist_find(), "hist_rects"))
        # (read-only passes: "bytes" counts the input twice so that the copy beside them moves as many bytes as they read)
        record("stats", dtype, bands, 2 * in_b, lambda: im.stats(), "stats_stream", against)
        del im, im2
        lib.vips_hip_pool_trim()
    lib.vips_hip_event_free(e0)
    lib.vips_hip_event_free(e1)
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "arith_times.json")
    with open(out, "w") as f:
        json.dump({"side": SIDE, "warm": WARM, "timed": TIMED, "window_ms": WINDOW_MS, "repeats": REPEATS, "peak_bytes_s": PEAK,
                   "rows": rows}, f, indent=1)
        f.write("\n")
    print("PERF-OK " + out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
