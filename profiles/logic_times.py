"""What the mask operations cost (libvips_amd/csrc/logic.hip, ops_logic.cpp) beside a device-to-device copy of the same
bytes, in ONE process on images resident on the device, at two sizes: SIDE x SIDE pels (8192) and 2 SIDE x 2 SIDE, where
every case moves more than 256 MiB, so that the Infinity Cache does not flatter the figure.

  more_const on uchar, ushort and float; more and `and` of two uchar images; ifthenelse of a one-band uchar mask over RGB
  uchar and over one-band float images (plain) and over one-band uchar images (blend); bandjoin of 3 + 1 uchar bands;
  extract_band of 1 of 4 uchar bands; bandmean of 3 uchar bands.

Every figure is device events on the library's stream round a window of calls after WARM, taken REPEATS times; the
median is reported and the spread kept.  A window holds as many calls as make it at least WINDOW_MS long (and at least
TIMED), counted from a first short window.  Every call is a Python call and a pool allocation of its result, so beside
the device time of a call the script keeps the HOST time the loop took to queue it (enqueue_ms): where that is below
the device time the queue never ran dry and the figure is the kernel's; a case where it is not is marked "host-bound"
and its figure is an upper bound of the kernel's time.  Bytes are the algorithm's: every input once plus the output
once.  The yardstick is vips_hip_memcpy_d2d of half those bytes (a copy reads and writes each of its bytes), timed the
same way; to_copy = the copy's time over the case's (1 = as fast as the copy).  hbm = bytes / time over 8 TB/s.
Usage: logic_times.py [output.json]   (LOGIC_PERF_SCALE=8 shrinks every side, for a rehearsal).  Needs the GPU: there is
no fallback."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCALE = int(os.environ.get("LOGIC_PERF_SCALE", "1"))
SIDES = (8192 // SCALE, 16384 // SCALE)
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

    def record(side, name, dtype, bands, nbytes, fn, kernel, against=None):
        ms, runs, calls, host = timed(fn)
        c_ms, c_runs, c_calls, c_host = copy_ms(nbytes)
        rate = nbytes / (ms * 1e-3)
        row = {"side": side, "case": name, "format": np.dtype(dtype).name, "bands": bands, "kernel": kernel, "bytes": nbytes, "ms": ms,
               "ms_runs": runs, "calls": calls, "enqueue_ms": host, "host_bound": host >= ms, "gb_s": rate / 1e9,
               "hbm": rate / PEAK, "copy_ms": c_ms, "copy_ms_runs": c_runs, "copy_calls": c_calls, "copy_enqueue_ms": c_host,
               "copy_host_bound": c_host >= c_ms, "to_copy": c_ms / ms}
        if against:
            row["against"], row["against_ms"] = against
            row["to_against"] = against[1] / ms
        rows.append(row)
        print("%5d  %-30s %-7s x%d  %8.3f ms (%5d calls, queued in %.3f ms each%s)  %8.1f GB/s  %5.1f %% of 8 TB/s   copy %8.3f ms   "
              "to_copy %.2f%s" % (side, name, np.dtype(dtype).name, bands, ms, calls, host, ", HOST-BOUND" if host >= ms else "",
                                  rate / 1e9, 100 * rate / PEAK, c_ms, c_ms / ms,
                                  "   %s %.3f ms, ratio %.2f" % (against[0], against[1], against[1] / ms) if against else ""), flush=True)
        return ms

    rng = np.random.default_rng(7)

    def image(side, bands, dtype, interp="multiband"):
        """Noise (a block of rows repeated down the image: the values do not matter to the time, the upload does)."""
        block = rng.integers(0, 256, (min(side, 512), side, bands), dtype=np.uint8).astype(dtype)
        return Image.new_from_array(np.tile(block, (side // block.shape[0], 1, 1)), interp)

    def gate_of(fn):
        lib.vips_hip_gate_reset()
        lib.vips_hip_gate_enable(1)
        try:
            fn()
            libvips_amd.synchronize()
            ran = sorted(k for k in libvips_amd.gate_report() if k.startswith("logic_"))
        finally:
            lib.vips_hip_gate_enable(0)
            lib.vips_hip_gate_reset()
        return "+".join(ran)

    for side in SIDES:
        pels = side * side
        for dtype in (np.uint8, np.uint16, np.float32):
            im = image(side, 1, dtype)
            fn = lambda: im.more(128)  # noqa: E731
            record(side, "more_const", dtype, 1, pels * (np.dtype(dtype).itemsize + 1), fn, gate_of(fn))
            del im
            lib.vips_hip_pool_trim()
        a, b = image(side, 1, np.uint8), image(side, 1, np.uint8)
        fn = lambda: a.more(b)  # noqa: E731
        record(side, "more", np.uint8, 1, pels * 3, fn, gate_of(fn))
        fn = lambda: a.andimage(b)  # noqa: E731
        record(side, "and", np.uint8, 1, pels * 3, fn, gate_of(fn))
        mask = image(side, 1, np.uint8)
        fn = lambda: mask.ifthenelse(a, b, blend=True)  # noqa: E731
        record(side, "ifthenelse blend", np.uint8, 1, pels * 4, fn, gate_of(fn))
        del b
        rgb, rgb2 = image(side, 3, np.uint8, "srgb"), image(side, 3, np.uint8, "srgb")
        fn = lambda: mask.ifthenelse(rgb, rgb2)  # noqa: E731
        record(side, "ifthenelse, mask over RGB", np.uint8, 3, pels * 10, fn, gate_of(fn))
        del rgb2
        fn = lambda: rgb.bandjoin(mask)  # noqa: E731
        record(side, "bandjoin 3 + 1", np.uint8, 4, pels * 8, fn, gate_of(fn))
        fn = lambda: rgb.bandmean()  # noqa: E731
        record(side, "bandmean of 3", np.uint8, 3, pels * 4, fn, gate_of(fn))
        del rgb
        lib.vips_hip_pool_trim()
        rgba = image(side, 4, np.uint8, "srgb")
        fn = lambda: rgba.extract_band(1)  # noqa: E731
        record(side, "extract_band 1 of 4", np.uint8, 4, pels * 5, fn, gate_of(fn))
        del rgba
        lib.vips_hip_pool_trim()
        fa, fb = image(side, 1, np.float32), image(side, 1, np.float32)
        fn = lambda: mask.ifthenelse(fa, fb)  # noqa: E731
        record(side, "ifthenelse", np.float32, 1, pels * 13, fn, gate_of(fn))
        del fa, fb, mask, a
        lib.vips_hip_pool_trim()
    lib.vips_hip_event_free(e0)
    lib.vips_hip_event_free(e1)
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "logic_times.json")
    with open(out, "w") as f:
        json.dump({"sides": SIDES, "warm": WARM, "timed": TIMED, "window_ms": WINDOW_MS, "repeats": REPEATS, "peak_bytes_s": PEAK,
                   "rows": rows}, f, indent=1)
        f.write("\n")
    print("PERF-OK " + out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
