"""What the general transform costs (libvips_amd/csrc/affine.hip), on 8192 x 8192 uchar images of 3 bands and of 4 (srgb
with alpha: the premultiply -> affine -> unpremultiply -> cast chain):

  * the floor: rot by 90 degrees of the same image, a transform that only moves bytes;
  * rotate 30 with each interpolator, similarity scale 0.5 angle 30 bicubic, affine with a pure shear (bilinear).

Every case is a process of its own under `timeout` (the parent stops at the first one that fails) and reports: ms a
call (device events on the library's stream round TIMED calls after WARM), the algorithmic bytes (input + output, once
each) over that time as a fraction of 8 TB/s, the ratio to the floor measured in the same run on the same image, the
kernels that ran (gate report), and the reference's time for the same call on the host cores (Ref.time_chain: graph
build + full evaluation into memory, best of 2) with the speed-up.  There is no pass bar.
Usage: time_affine.py [output file]   (AFFINE_PERF_SCALE=8 shrinks every side, for a rehearsal;
AFFINE_PERF_REF=0 leaves the reference out)"""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCALE = int(os.environ.get("AFFINE_PERF_SCALE", "1"))
WITH_REF = os.environ.get("AFFINE_PERF_REF", "1") != "0"
SIDE = 8192 // SCALE
WARM, TIMED = 2, 5
PEAK = 8e12
STEP_SECONDS = 240
SRGB = 22

# (name, operation, arguments of Image.<operation>, the reference's chain)
OPS = [
    ("rot d90 (floor)", "rot", dict(angle="d90"), "rot:angle=d90"),
    ("rotate 30 nearest", "rotate", dict(angle=30, interpolate="nearest"), "rotate:angle=30,interpolate=nearest"),
    ("rotate 30 bilinear", "rotate", dict(angle=30, interpolate="bilinear"), "rotate:angle=30,interpolate=bilinear"),
    ("rotate 30 bicubic", "rotate", dict(angle=30, interpolate="bicubic"), "rotate:angle=30,interpolate=bicubic"),
    ("similarity 0.5 30 bicubic", "similarity", dict(scale=0.5, angle=30, interpolate="bicubic"),
     "similarity:scale=0.5,angle=30,interpolate=bicubic"),
    ("affine shear 1 0.3 0 1", "affine", dict(matrix=(1, 0.3, 0, 1)), "affine:matrix=1 0.3 0 1"),
]
CASES = [(bands, op) for bands in (3, 4) for op in OPS]


def one_case(number):
    import libvips_amd
    from libvips_amd import Image, _ffi
    from tests import helpers
    from tests.helpers import Ref

    lib = _ffi.lib
    libvips_amd.init(0)
    bands, (name, op, kw, chain) = CASES[number]
    interpretation = SRGB if bands == 4 else 0
    src = helpers.lcg_image(SIDE, SIDE, bands, np.uint8, 5)
    im = Image.new_from_array(src, interpretation=interpretation)
    fn = lambda: getattr(im, op)(**kw)  # noqa: E731

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
    nbytes = src.nbytes + out.width * out.height * out.bands

    ref_ms = float("nan")
    if WITH_REF and helpers.have_ref():
        ref_ms = Ref.time_chain(chain, src, repeats=2, interpretation=interpretation) * 1e3
    kernels = "  ".join("%s x%d %.3f" % (k, n, t) for k, (n, t) in sorted(report.items()))
    print("RESULT\t%d bands: %s\t%.4f\t%d\t%.1f\t%s" % (bands, name, ms, nbytes, ref_ms, kernels), flush=True)


def main():
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say("# %d x %d uchar; %d warm-up + %d timed calls a case, device events round the timed calls; a process a case" % (
        SIDE, SIDE, WARM, TIMED))
    say("# %-36s %9s %8s %8s %11s %8s   kernels (gate: launches ms)" % ("case", "ms", "% 8TB/s", "x rot90", "ref ms", "ref / us"))
    floor = {}
    for number, (bands, op) in enumerate(CASES):
        proc = subprocess.run(["timeout", "-k", "10", str(STEP_SECONDS), sys.executable, os.path.abspath(__file__), "--case", str(number)],
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        result = [l for l in proc.stdout.splitlines() if l.startswith("RESULT\t")]
        if proc.returncode != 0 or not result:
            say("FAILED %d bands: %s (exit %d): %s" % (bands, op[0], proc.returncode, proc.stdout[-2000:]))
            return 1
        _, name, ms, nbytes, ref_ms, kernels = result[0].split("\t")
        ms, nbytes, ref_ms = float(ms), int(nbytes), float(ref_ms)
        floor.setdefault(bands, ms)
        say("  %-36s %9.3f %8.1f %8.2f %11.1f %8.0f   %s" % (name, ms, nbytes / (ms * 1e-3) / PEAK * 100, ms / floor[bands], ref_ms,
                                                           ref_ms / ms, kernels))
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
