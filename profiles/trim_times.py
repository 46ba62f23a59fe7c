"""What project, profile and find_trim cost (libvips_amd/csrc/trim.hip, ops_trim.cpp) beside the read-only passes the
library already had, in ONE process on a uchar RGB image resident on the device, at two sizes: SIDE x SIDE pels (8192,
201 MB) and 2 SIDE x 2 SIDE (805 MB, past the 256 MiB Infinity Cache).

  a device-to-device copy of the image; stats and hist_find (read-only passes); median(3) alone (one link of find_trim's
  chain: reads and writes the image); project; profile; find_trim on the composed route (VIPS_HIP_NO_TRIM_FUSED) and on
  the fused one.

The image is a scan: a white page with a rectangle of noise on it, so that find_trim has something to find.  Every
figure is device events on the library's stream round a window of calls after WARM, taken REPEATS times; the median is
reported, every repeat kept, and spread = max - min of the repeats.  A window holds as many calls as make it at least
WINDOW_MS long (and at least TIMED).  kernel_ms is each kernel alone, by the gates' own events over GATED more calls.  stats, hist_find's consumers aside, and find_trim end in a copy to the host, so
their figure is the whole call: kernel, copy and the host's finish.  The comparisons the figures are for, each with a
margin equal to the spread of the side compared against:
  project against stats (the same bytes read); fused find_trim against median(3) alone; fused against composed.
Usage: trim_times.py [output.json]   (TRIM_PERF_SCALE=8 shrinks every side, for a rehearsal).  Needs the GPU: there is no
fallback."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCALE = int(os.environ.get("TRIM_PERF_SCALE", "1"))
SIDES = (8192 // SCALE, 16384 // SCALE)
WARM, TIMED, REPEATS = 3, 10, 5
WINDOW_MS = 200.0
GATED = 20
PEAK = 8e12


def main():
    import libvips_amd
    from libvips_amd import Image, _ffi

    lib = _ffi.lib
    libvips_amd.init(0)
    e0, e1 = lib.vips_hip_event_new(), lib.vips_hip_event_new()
    assert e0 and e1

    def window(fn, calls):
        """-> (device ms a call, host ms a call)"""
        _ffi.check(lib.vips_hip_event_record(e0))
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        host = (time.perf_counter() - t0) * 1e3 / calls
        _ffi.check(lib.vips_hip_event_record(e1))
        _ffi.check(lib.vips_hip_event_synchronize(e1))
        return lib.vips_hip_event_elapsed_ms(e0, e1) / calls, host

    def timed(fn):
        for _ in range(WARM):
            fn()
        libvips_amd.synchronize()
        first, _ = window(fn, TIMED)
        calls = max(TIMED, int(WINDOW_MS / max(first, 1e-3)) + 1) if first > 0 else TIMED  # (events that do not tick: a rehearsal)
        runs = [window(fn, calls) for _ in range(REPEATS)]
        ms = [r[0] for r in runs]
        # (a runtime whose events do not tick -- the CPU suite's mock -- must not divide by zero)
        return {"ms": max(float(np.median(ms)), 1e-6), "ms_runs": ms, "spread_ms": max(ms) - min(ms), "calls": calls,
                "host_ms": float(np.median([r[1] for r in runs]))}

    def gates(fn):
        """-> ({gate: launches of one call}, {gate: ms a launch, by the gate's own events, over GATED calls}): the kernels
        alone, apart from the copies, the allocations and the host's share of a call"""
        lib.vips_hip_gate_reset()
        lib.vips_hip_gate_enable(1)
        try:
            for _ in range(GATED):
                fn()
            libvips_amd.synchronize()
            report = libvips_amd.gate_report()
            return {k: n // GATED for k, (n, _) in report.items()}, {k: ms / max(n, 1) for k, (n, ms) in report.items()}
        finally:
            lib.vips_hip_gate_enable(0)
            lib.vips_hip_gate_reset()

    rng = np.random.default_rng(11)
    rows, comparisons = [], []
    for side in SIDES:
        page = np.full((side, side, 3), 255, np.uint8)
        block = rng.integers(0, 256, (min(side, 512), side * 3 // 4, 3), dtype=np.uint8)
        top, left = side // 10, side // 8
        page[top:top + (side * 7 // 10) // block.shape[0] * block.shape[0], left:left + block.shape[1]] = np.tile(
            block, ((side * 7 // 10) // block.shape[0], 1, 1))
        im = Image.new_from_array(page, "srgb")
        nbytes = page.nbytes
        del page
        spare = lib.vips_hip_malloc(nbytes)
        assert spare

        def composed():
            os.environ["VIPS_HIP_NO_TRIM_FUSED"] = "1"
            try:
                return im.find_trim()
            finally:
                del os.environ["VIPS_HIP_NO_TRIM_FUSED"]

        cases = [("copy", lambda: _ffi.check(lib.vips_hip_memcpy_d2d(spare, lib.vips_hip_image_get_data(im._h), nbytes)), 2 * nbytes),
                 ("stats", im.stats, nbytes), ("hist_find", im.hist_find, nbytes), ("median3", lambda: im.median(3), 2 * nbytes),
                 ("project", im.project, nbytes), ("profile", im.profile, nbytes), ("find_trim composed", composed, 17 * nbytes),
                 ("find_trim fused", im.find_trim, nbytes)]
        assert composed() == im.find_trim()
        by_name = {}
        for name, fn, moved in cases:
            t = timed(fn)
            ran, kernel_ms = gates(fn) if name != "copy" else ({}, {})
            row = dict(t, side=side, case=name, bytes_moved=moved, gates=ran, kernel_ms=kernel_ms, gb_s=moved / (t["ms"] * 1e-3) / 1e9,
                       hbm=moved / (t["ms"] * 1e-3) / PEAK, image_gb_s=nbytes / (t["ms"] * 1e-3) / 1e9)
            rows.append(row)
            by_name[name] = row
            print("%5d  %-20s %9.3f ms  (spread %.3f, %d calls, host %.3f ms a call)  image at %7.1f GB/s   %s" % (
                side, name, t["ms"], t["spread_ms"], t["calls"], t["host_ms"], row["image_gb_s"],
                " + ".join("%s %.3f" % (k, kernel_ms[k]) for k in sorted(ran))), flush=True)
        for a, b in (("project", "stats"), ("find_trim fused", "median3"), ("find_trim fused", "find_trim composed")):
            ra, rb = by_name[a], by_name[b]
            c = {"side": side, "what": a, "against": b, "ms": ra["ms"], "against_ms": rb["ms"], "margin_ms": rb["spread_ms"],
                 "ratio": rb["ms"] / ra["ms"], "not_slower": ra["ms"] <= rb["ms"] + rb["spread_ms"]}
            comparisons.append(c)
            print("%5d  %s %.3f ms against %s %.3f ms +- %.3f: %s (%.2fx)" % (
                side, a, c["ms"], b, c["against_ms"], c["margin_ms"], "not slower" if c["not_slower"] else "SLOWER", c["ratio"]), flush=True)
        lib.vips_hip_free(spare)
        del im
        lib.vips_hip_pool_trim()
    lib.vips_hip_event_free(e0)
    lib.vips_hip_event_free(e1)
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "trim_times.json")
    with open(out, "w") as f:
        json.dump({"sides": SIDES, "warm": WARM, "timed": TIMED, "window_ms": WINDOW_MS, "repeats": REPEATS, "peak_bytes_s": PEAK,
                   "rows": rows, "comparisons": comparisons}, f, indent=1)
        f.write("\n")
    print("PERF-OK " + out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
