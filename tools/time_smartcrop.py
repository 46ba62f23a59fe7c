"""What the content-driven crops cost (libvips_amd/csrc/hist.hip, attention.hip, smartcrop.cpp), on an 8192 x 8192 x 3
uchar image (201 MB: it sits INSIDE the 256 MB Infinity Cache, so the histogram kernel's rate below is not an HBM rate):

  * thumbnail_image -> 256 x 256 and -> 256 x 160 with crop=centre, entropy and attention: the two differences
    from centre are the feature's cost on a thumbnail (the crop works on the finished thumbnail, 256 x 256 pels: for
    the square box there is nothing to trim, for the other one 96 rows go);
  * smartcrop -> 4096 x 4096 for both modes, beside the reference's wall time for the same call on the host cores;
  * for the entropy search: launches of the histogram kernel (gate report), copies back (one per launch, by the
    code), and the kernel's bytes over its gate time for the six slices of the search's first round, for the
    whole image (a quiet picture: lanes of a wave meet on few bins) and for a whole image of noise (they rarely meet).

Calls are timed with device events on the library's stream round TIMED calls after WARM (the calls copy their
decisions back, so the events enclose those waits), kernels by their gates.  Usage: time_smartcrop.py [output file]
(SMARTCROP_PERF_SCALE=8 shrinks every side, for a rehearsal)"""
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import libvips_amd  # noqa: E402
from libvips_amd import Image, _ffi  # noqa: E402
from tests import helpers  # noqa: E402
from tests.helpers import Ref  # noqa: E402

SCALE = int(os.environ.get("SMARTCROP_PERF_SCALE", "1"))
WARM, TIMED = 3, 10
lib = _ffi.lib
libvips_amd.init(0)
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def event_ms(fn):
    """ms a call, by events on the library's stream round TIMED calls after WARM."""
    for _ in range(WARM):
        fn()
    libvips_amd.synchronize()
    e0, e1 = lib.vips_hip_event_new(), lib.vips_hip_event_new()
    assert e0 and e1
    try:
        _ffi.check(lib.vips_hip_event_record(e0))
        for _ in range(TIMED):
            fn()
        _ffi.check(lib.vips_hip_event_record(e1))
        _ffi.check(lib.vips_hip_event_synchronize(e1))
        return lib.vips_hip_event_elapsed_ms(e0, e1) / TIMED
    finally:
        lib.vips_hip_event_free(e0)
        lib.vips_hip_event_free(e1)


def gates(fn, calls=1):
    """{gate: (launches, ms)} of `calls` calls (after the warm-up event_ms gave them)."""
    libvips_amd.synchronize()
    lib.vips_hip_gate_reset()
    lib.vips_hip_gate_enable(1)
    try:
        for _ in range(calls):
            fn()
        libvips_amd.synchronize()
        return libvips_amd.gate_report()
    finally:
        lib.vips_hip_gate_enable(0)
        lib.vips_hip_gate_reset()


SIDE = 8192 // SCALE
BANDS = 3
# a quiet gradient with noise on top and one busy disc: the searches have something to find
xs, ys = np.arange(SIDE), np.arange(SIDE)[:, None]
base = ((xs * 40) // SIDE).astype(np.uint8)[None, :] + ((ys * 30) // SIDE + 60).astype(np.uint8)
src = helpers.lcg_image(SIDE, SIDE, BANDS, np.uint8, 5) // 32 + base[..., None]
disc = ((xs - 3 * SIDE // 4) ** 2)[None, :] + (ys - 2 * SIDE // 3) ** 2 < (SIDE // 8) ** 2
src[disc] = helpers.lcg_image(SIDE, SIDE, BANDS, np.uint8, 6)[disc]
del xs, ys, base, disc
im = Image.new_from_array(src, interpretation="srgb")
say("# %d x %d x %d uchar (%.0f MB); %d warm-up + %d timed calls, device events round the timed calls" % (
    SIDE, SIDE, BANDS, src.nbytes / 1e6, WARM, TIMED))

say("")
for tw, th in ((256 // SCALE, 256 // SCALE), (256 // SCALE, 160 // SCALE)):
    say("## thumbnail_image -> %d x %d%s" % (tw, th, "" if tw != th else "   (the thumbnail fills the box: nothing to trim)"))
    base = None
    for crop in ("centre", "entropy", "attention"):
        ms = event_ms(lambda: im.thumbnail_image(tw, th, crop=crop))
        base = ms if base is None else base
        report = gates(lambda: im.thumbnail_image(tw, th, crop=crop))
        mine = {k: v for k, v in report.items() if k.startswith("hist_") or k.startswith("attention_")}
        say("  crop=%-10s %9.3f ms   %+9.3f ms over centre   %s" % (crop, ms, ms - base, "  ".join(
            "%s x%d %.3f ms" % (k, n, t) for k, (n, t) in sorted(mine.items()))))
say("")
say("## smartcrop -> %d x %d" % (SIDE // 2, SIDE // 2))
C = SIDE // 2
ref_path = None
if helpers.have_ref():
    ref_path = os.path.join(tempfile.mkdtemp(prefix="smartcrop_perf_"), "in.v")
    helpers.write_v(ref_path, src)
for mode in ("entropy", "attention"):
    ms = event_ms(lambda: im.smartcrop(C, C, interesting=mode))
    _, opts = im.smartcrop(C, C, interesting=mode, with_options=True)
    report = gates(lambda: im.smartcrop(C, C, interesting=mode))
    text = "  %-10s %9.3f ms   at (%d, %d)" % (mode, ms, opts["left"], opts["top"])
    if mode == "entropy":
        n, t = report["hist_rects"]
        text += "   hist_rects: %d launches, %d copies back (one a launch), %.3f ms in the kernel" % (n, n, t)
    say(text)
    if ref_path:
        args = "input=%s,width=%d,height=%d,interesting=%s" % (ref_path, C, C, mode)
        Ref.create("smartcrop", args)  # (the file is in the page cache after this)
        t0 = time.perf_counter()
        want, _, _ = Ref.create("smartcrop", args)
        ref_ms = (time.perf_counter() - t0) * 1e3
        same = np.array_equal(want, im.smartcrop(C, C, interesting=mode).numpy())
        say("  %-10s %9.1f ms   reference, host cores (%d threads), wall time with the .v file mapped; same crop: %s" % (
            "", ref_ms, Ref.concurrency(), same))
if ref_path:
    os.remove(ref_path)
    os.rmdir(os.path.dirname(ref_path))

say("")
say("## the histogram kernel (gate time; bytes = the pels counted)")
S = SIDE // 16  # the slice of the search's first round to SIDE / 2
first_round = [(0, 0, S, SIDE), (SIDE - S, 0, S, SIDE), (0, 0, SIDE - S, S), (0, SIDE - S, SIDE - S, S),
               (S, 0, SIDE - S, S), (S, SIDE - S, SIDE - S, S)]
whole = [(0, 0, SIDE, SIDE)]
plain = Image.new_from_array(helpers.lcg_image(SIDE, SIDE, BANDS, np.uint8, 7))
for name, image, rects in (("six slices of round 1", im, first_round), ("the whole image", im, whole),
                           ("a whole image of noise", plain, whole)):
    event_ms(lambda: image.hist_rects(rects))
    n, t = gates(lambda: image.hist_rects(rects), TIMED)["hist_rects"]
    nbytes = sum(w * h * BANDS for _, _, w, h in rects)
    ms = max(t / n, 1e-9)
    say("  %-24s %9.3f ms   %7.1f MB   %8.1f GB/s" % (name, ms, nbytes / 1e6, nbytes / ms / 1e6))
say("PERF-OK")
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
