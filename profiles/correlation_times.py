"""What fastcor and spcor cost (libvips_amd/csrc/correlation.hip), in ONE process on a SIDE x SIDE image resident on the
device (4096), one band and three, with 16 x 16 and 64 x 64 refs:

  (a) fastcor of uchar, beside conv of the same image with an integer mask of the ref's size (precision integer): both
      do one multiply-add a tap an element;
  (b) spcor of uchar, beside the float conv of that size: spcor does five unfused double operations a tap (and a pass of
      double additions before them) where conv does one fused multiply-add;
  (c) fastcor of float, beside the same float conv of the float image;
  (d) the reference's own `vips fastcor` / `vips spcor` at its full concurrency on the same pixels through .v files
      (wall time of the command, the files' reading and writing included), where oracle/_ref is built: the CPU figure.
      The 64 x 64 refs are run on one band only.

The yardsticks are code that was there before.  No ratio is asserted: times and ratios are recorded.  Every device figure
is device events on the library's stream round a window of calls after WARM, taken REPEATS times; the median is
reported, every repeat kept, and spread = max - min of the repeats.  A window holds as many calls as make it at least
WINDOW_MS long (and at least TIMED).
Usage: correlation_times.py [output.json]   (CORRELATION_PERF_SCALE=8 shrinks the side, for a rehearsal).  Needs the GPU:
there is no fallback."""
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCALE = int(os.environ.get("CORRELATION_PERF_SCALE", "1"))
SIDE = 4096 // SCALE
WARM, TIMED, REPEATS = 2, 3, 5
WINDOW_MS = 200.0
REFS = (16, 64)
BANDS = (1, 3)


def main():
    import libvips_amd
    from libvips_amd import Image, _ffi
    from tests import helpers

    lib = _ffi.lib
    libvips_amd.init(0)
    e0, e1 = lib.vips_hip_event_new(), lib.vips_hip_event_new()
    assert e0 and e1

    def window(fn, calls):
        _ffi.check(lib.vips_hip_event_record(e0))
        for _ in range(calls):
            fn()
        _ffi.check(lib.vips_hip_event_record(e1))
        _ffi.check(lib.vips_hip_event_synchronize(e1))
        return lib.vips_hip_event_elapsed_ms(e0, e1) / calls

    def timed(fn):
        for _ in range(WARM):
            fn()
        libvips_amd.synchronize()
        first = window(fn, TIMED)
        calls = max(TIMED, int(WINDOW_MS / max(first, 1e-3)) + 1) if first > 0 else TIMED  # (events that do not tick: a rehearsal)
        ms = [window(fn, calls) for _ in range(REPEATS)]
        return {"ms": max(float(np.median(ms)), 1e-6), "ms_runs": ms, "spread_ms": max(ms) - min(ms), "calls": calls}

    vips = os.path.join(ROOT, "oracle", "_ref", "bin", "vips")
    tmp = tempfile.mkdtemp(prefix="correlation_times_")

    def cpu_ms(op, im, ref):
        """The reference's command at its default (full) concurrency: the best of two."""
        if not os.path.exists(vips):
            return None
        a, b, o = (os.path.join(tmp, n) for n in ("in.v", "ref.v", "out.v"))
        helpers.write_v(a, im, 0)
        helpers.write_v(b, ref, 0)
        env = helpers.ref_cli_env()
        env.pop("VIPS_CONCURRENCY", None)
        best = None
        for _ in range(2):
            t0 = time.perf_counter()
            subprocess.run([vips, op, a, b, o], env=env, check=True)
            t = (time.perf_counter() - t0) * 1e3
            best = t if best is None else min(best, t)
        for p in (a, b, o):
            os.remove(p)
        return best

    rng = np.random.default_rng(17)
    rows = []
    for bands in BANDS:
        u8 = rng.integers(0, 256, (SIDE, SIDE, bands), dtype=np.uint8)
        f32 = ((rng.random((SIDE, SIDE, bands)) - 0.5) * 600.0).astype(np.float32)
        dev_u8, dev_f32 = Image.new_from_array(u8), Image.new_from_array(f32)
        for side in REFS:
            ref_u8 = np.ascontiguousarray(u8[100 // SCALE:100 // SCALE + side, 200 // SCALE:200 // SCALE + side])
            ref_f32 = np.ascontiguousarray(f32[100 // SCALE:100 // SCALE + side, 200 // SCALE:200 // SCALE + side])
            dref_u8, dref_f32 = Image.new_from_array(ref_u8), Image.new_from_array(ref_f32)
            imask = rng.integers(-8, 9, (side, side)).astype(np.float64)
            fmask = rng.random((side, side)) - 0.5
            taps = float(SIDE) * SIDE * bands * side * side
            cases = [
                ("fastcor uchar", lambda: dev_u8.fastcor(dref_u8), "conv integer", lambda: dev_u8.conv(imask, precision="integer"),
                 ("fastcor", u8, ref_u8)),
                ("spcor uchar", lambda: dev_u8.spcor(dref_u8), "conv float", lambda: dev_u8.conv(fmask, precision="float"),
                 ("spcor", u8, ref_u8)),
                ("fastcor float", lambda: dev_f32.fastcor(dref_f32), "conv float of float", lambda: dev_f32.conv(fmask, precision="float"),
                 ("fastcor", f32, ref_f32)),
            ]
            for name, fn, yard_name, yard_fn, cpu in cases:
                t = timed(fn)
                try:
                    y = timed(yard_fn)
                except _ffi.VipsHipError as e:  # (a mask the convolution does not take: recorded, not hidden)
                    print("%s %d x %d: %s" % (yard_name, side, side, e), flush=True)
                    y = {"ms": None, "spread_ms": None, "ms_runs": []}
                c = cpu_ms(*cpu) if (side == REFS[0] or bands == 1) else None
                row = {"case": name, "bands": bands, "ref": side, "taps": taps, "ms": t["ms"], "spread_ms": t["spread_ms"],
                       "ms_runs": t["ms_runs"], "calls": t["calls"], "gtaps_per_s": taps / (t["ms"] * 1e-3) / 1e9,
                       "yardstick": yard_name, "yardstick_ms": y["ms"], "yardstick_spread_ms": y["spread_ms"],
                       "yardstick_ms_runs": y["ms_runs"], "ratio_to_yardstick": None if y["ms"] is None else t["ms"] / y["ms"],
                       "reference_cpu_ms": c, "reference_cpu_over_device": None if c is None else c / t["ms"]}
                rows.append(row)
                print("%-14s %d band  ref %2d  %9.3f ms (spread %.3f, %d calls, %7.1f Gtap/s)  %-19s %9.3f ms  ratio %5.2f  cpu %s" % (
                    name, bands, side, t["ms"], t["spread_ms"], t["calls"], row["gtaps_per_s"], yard_name, y["ms"] or 0.0,
                    row["ratio_to_yardstick"] or 0.0, "-" if c is None else "%.0f ms" % c), flush=True)
        del dev_u8, dev_f32
    lib.vips_hip_event_free(e0)
    lib.vips_hip_event_free(e1)
    os.rmdir(tmp)
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "correlation_times.json")
    with open(out, "w") as f:
        json.dump({"side": SIDE, "warm": WARM, "timed": TIMED, "window_ms": WINDOW_MS, "repeats": REPEATS, "rows": rows}, f, indent=1)
        f.write("\n")
    print("PERF-OK " + out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
