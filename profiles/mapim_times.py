"""What mapim costs (libvips_amd/csrc/mapim.hip) beside the gather the library already had, in ONE process on a SIDE x SIDE
uchar RGB image resident on the device (8192: 201 MB), under nearest, bilinear and bicubic:

  (a) affine with a 30 degree rotation, its output area a SIDE x SIDE window in the middle of the rotated image;
  (b) mapim through a float index that holds that rotation's coordinates for the same window (537 MB at 8192);
  (c) mapim through the identity index Image.xyz makes (uint, as many bytes);
  (d) a device-to-device copy of the index's bytes.

The yardstick for (b) is (a) + (d), both of them code that was there before: mapim does affine's gather plus one read of
the index.  Every figure is device events on the library's stream round a window of calls after WARM, taken REPEATS
times; the median is reported, every repeat kept, and spread = max - min of the repeats.  A window holds as many calls as
make it at least WINDOW_MS long (and at least TIMED).  (a) and (b) do not make the same bytes -- affine accumulates its
coordinates in double, the index holds floats -- so the share of pels on which they agree is reported, not asserted.
Usage: mapim_times.py [output.json]   (MAPIM_PERF_SCALE=8 shrinks the side, for a rehearsal).  Needs the GPU: there is
no fallback."""
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCALE = int(os.environ.get("MAPIM_PERF_SCALE", "1"))
SIDE = 8192 // SCALE
ANGLE = 30.0
WARM, TIMED, REPEATS = 3, 5, 5
WINDOW_MS = 200.0
INTERPOLATORS = ("nearest", "bilinear", "bicubic")


def main():
    import libvips_amd
    from libvips_amd import Image, _ffi

    lib = _ffi.lib
    libvips_amd.init(0)
    e0, e1 = lib.vips_hip_event_new(), lib.vips_hip_event_new()
    assert e0 and e1

    def window(fn, calls):
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
        return {"ms": max(float(np.median(ms)), 1e-6), "ms_runs": ms, "spread_ms": max(ms) - min(ms), "calls": calls,
                "host_ms": float(np.median([r[1] for r in runs]))}

    rng = np.random.default_rng(11)
    im = Image.new_from_array(rng.integers(0, 256, (SIDE, SIDE, 3), dtype=np.uint8))
    # vips_rotate's matrix (similarity.c:83-111) and the middle SIDE x SIDE of the rotated image's bounding box
    rad = ANGLE / 360.0 * 2.0 * math.pi
    a, b, c, d = math.cos(rad), -math.sin(rad), math.sin(rad), math.cos(rad)
    xs = [a * x + b * y for x in (0, SIDE) for y in (0, SIDE)]
    ys = [c * x + d * y for x in (0, SIDE) for y in (0, SIDE)]
    left = int(round(min(xs))) + (int(round(max(xs) - min(xs))) - SIDE) // 2
    top = int(round(min(ys))) + (int(round(max(ys) - min(ys))) - SIDE) // 2
    oarea = (left, top, SIDE, SIDE)
    # the inverse's coordinates of that window, as the floats of an index
    det = a * d - b * c
    ia, ib, ic, id_ = d / det, -b / det, -c / det, a / det
    ox = (np.arange(SIDE, dtype=np.float64) + left)[None, :]
    oy = (np.arange(SIDE, dtype=np.float64) + top)[:, None]
    index = np.empty((SIDE, SIDE, 2), np.float32)
    index[:, :, 0] = ia * ox + ib * oy
    index[:, :, 1] = ic * ox + id_ * oy
    rotation = Image.new_from_array(index)
    index_bytes = index.nbytes
    del index
    identity = Image.xyz(SIDE, SIDE)
    spare = lib.vips_hip_malloc(index_bytes)
    assert spare
    out_bytes = SIDE * SIDE * 3

    rows, comparisons = [], []
    copy = timed(lambda: _ffi.check(lib.vips_hip_memcpy_d2d(spare, lib.vips_hip_image_get_data(rotation._h), index_bytes)))
    rows.append(dict(copy, case="copy of the index", interpolate=None, bytes_moved=2 * index_bytes))
    print("%-34s %9.3f ms  (spread %.3f, %d calls)  %7.1f GB/s" % ("(d) copy of the index", copy["ms"], copy["spread_ms"], copy["calls"],
                                                                    2 * index_bytes / (copy["ms"] * 1e-3) / 1e9), flush=True)
    for interpolate in INTERPOLATORS:
        cases = [("affine", lambda: im.affine((a, b, c, d), oarea=oarea, interpolate=interpolate)),
                 ("mapim rotation index", lambda: im.mapim(rotation, interpolate=interpolate)),
                 ("mapim identity index", lambda: im.mapim(identity, interpolate=interpolate))]
        agree = float((cases[0][1]().numpy() == cases[1][1]().numpy()).all(-1).mean())
        by_name = {}
        for name, fn in cases:
            t = timed(fn)
            row = dict(t, case=name, interpolate=interpolate, out_bytes=out_bytes, index_bytes=0 if name == "affine" else index_bytes)
            rows.append(row)
            by_name[name] = row
            print("%-10s %-23s %9.3f ms  (spread %.3f, %d calls, host %.3f ms a call)" % (
                interpolate, name, t["ms"], t["spread_ms"], t["calls"], t["host_ms"]), flush=True)
        ra, rb = by_name["affine"], by_name["mapim rotation index"]
        yard, margin = ra["ms"] + copy["ms"], ra["spread_ms"] + copy["spread_ms"]
        comp = {"interpolate": interpolate, "mapim_ms": rb["ms"], "affine_ms": ra["ms"], "copy_ms": copy["ms"], "yardstick_ms": yard,
                "margin_ms": margin, "within": rb["ms"] <= yard + margin, "pels_that_agree_with_affine": agree,
                "identity_ms": by_name["mapim identity index"]["ms"]}
        comparisons.append(comp)
        print("%-10s mapim %.3f ms against affine + copy %.3f ms +- %.3f: %s; %.4f of the pels agree with affine" % (
            interpolate, rb["ms"], yard, margin, "within" if comp["within"] else "BEYOND", agree), flush=True)
    lib.vips_hip_free(spare)
    lib.vips_hip_event_free(e0)
    lib.vips_hip_event_free(e1)
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "mapim_times.json")
    with open(out, "w") as f:
        json.dump({"side": SIDE, "angle": ANGLE, "warm": WARM, "timed": TIMED, "window_ms": WINDOW_MS, "repeats": REPEATS,
                   "rows": rows, "comparisons": comparisons}, f, indent=1)
        f.write("\n")
    print("PERF-OK " + out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
