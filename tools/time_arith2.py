"""What recomb, sum, bandrank, clamp and remainder_const cost (libvips_amd/csrc/recomb.hip, nary.hip, arith.hip), in one
process on 8192 x 8192 images resident on the device:

  * recomb 3 x 3 on uchar x 3 and on float x 3, 4 x 4 on uchar x 4 (the streaming kernel), 5 -> 2 on uchar (the general one);
  * sum and bandrank (the median) of three and of nine uchar x 3 images;
  * clamp and remainder_const on uchar x 3 and on float x 4.

Each is reported two ways: as a fraction of vips_hip_memcpy_d2d moving the same in + out bytes in this process (a copy of
half of them: it reads and writes each byte once), and beside the reference's time on the same machine's host cores
(Ref.time_chain; the command line on .v files for the operations on several images, which maps the files and writes the
result).  ms a call: device events on the library's stream round TIMED calls after WARM.
Usage: time_arith2.py [output file]   (ARITH2_PERF_SCALE=8 shrinks every side, for a rehearsal; ARITH2_PERF_REF=0 leaves
the reference out)"""
import ctypes
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCALE = int(os.environ.get("ARITH2_PERF_SCALE", "1"))
WITH_REF = os.environ.get("ARITH2_PERF_REF", "1") != "0"
SIDE = 8192 // SCALE
WARM, TIMED = 2, 8
SEPIA = [[0.393, 0.769, 0.189], [0.349, 0.686, 0.168], [0.272, 0.534, 0.131]]


def main():
    import libvips_amd
    from libvips_amd import Image, _ffi
    from tests import helpers
    from tests.helpers import Ref

    lib = _ffi.lib
    libvips_amd.init(0)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def timed(fn):
        for _ in range(WARM):
            fn()
        libvips_amd.synchronize()
        e0, e1 = lib.vips_hip_event_new(), lib.vips_hip_event_new()
        _ffi.check(lib.vips_hip_event_record(e0))
        for _ in range(TIMED):
            fn()
        _ffi.check(lib.vips_hip_event_record(e1))
        _ffi.check(lib.vips_hip_event_synchronize(e1))
        ms = lib.vips_hip_event_elapsed_ms(e0, e1) / TIMED
        lib.vips_hip_event_free(e0)
        lib.vips_hip_event_free(e1)
        return ms

    copies = {}

    def copy_ms(moved):
        """A device-to-device copy that moves `moved` bytes (reads half of them, writes half)."""
        half = moved // 2
        if half not in copies:
            src, dst = lib.vips_hip_malloc(half), lib.vips_hip_malloc(half)
            assert src and dst
            copies[half] = timed(lambda: _ffi.check(lib.vips_hip_memcpy_d2d(dst, src, half)))
            lib.vips_hip_free(src)
            lib.vips_hip_free(dst)
        return copies[half]

    def kernels(fn):
        lib.vips_hip_gate_reset()
        lib.vips_hip_gate_enable(1)
        fn()
        libvips_amd.synchronize()
        report = libvips_amd.gate_report()
        lib.vips_hip_gate_enable(0)
        lib.vips_hip_gate_reset()
        return ", ".join("%s x %d" % (k, n) for k, (n, _) in sorted(report.items()))

    noise = helpers.lcg_bytes(SIDE * SIDE * 5, 11)

    def image(dtype, bands, seed):
        """Seeded noise: one stream of bytes, turned by `seed` places (floats: 0 .. 1)."""
        a = np.roll(noise, 7919 * seed)[:SIDE * SIDE * bands].reshape(SIDE, SIDE, bands)
        return np.ascontiguousarray(a) if dtype == np.uint8 else (a.astype(np.float32) / np.float32(255.0))

    def report(name, fn, in_bytes, out_bytes, ref_ms):
        ms = timed(fn)
        cp = copy_ms(in_bytes + out_bytes)
        say("%-34s %8.3f ms  %7.1f GB/s of in + out  copy of the same bytes %8.3f ms  fraction of the copy %.2f  reference %9.1f ms (%.0f x)  [%s]" % (
            name, ms, (in_bytes + out_bytes) / (ms * 1e-3) / 1e9, cp, cp / ms, ref_ms, ref_ms / ms, kernels(fn)))

    def ref_chain(chain, array):
        if not (WITH_REF and helpers.have_ref()):
            return float("nan")
        return Ref.time_chain(chain, array, repeats=3) * 1e3

    say("# %d x %d images, resident; %d warm-up + %d timed calls each, device events round the timed calls; one process" % (SIDE, SIDE, WARM, TIMED))
    say("# the device's clocks as found: nothing sets or reads them; the reference (%d threads) on the same machine's host cores" % (
        Ref.concurrency() if WITH_REF and helpers.have_ref() else 0))
    n = SIDE * SIDE
    with tempfile.TemporaryDirectory() as tmp:
        def matrix_file(m):
            path = os.path.join(tmp, "m%dx%d.v" % (len(m[0]), len(m)))
            helpers.write_v(path, np.asarray(m, np.float64)[:, :, None], 0)
            return path

        # recomb
        rng = np.random.default_rng(3)
        for name, dtype, bands, m in (("recomb 3x3 uchar x 3", np.uint8, 3, SEPIA), ("recomb 3x3 float x 3", np.float32, 3, SEPIA),
                                      ("recomb 4x4 uchar x 4", np.uint8, 4, rng.normal(0, 1, (4, 4)).tolist()),
                                      ("recomb 5->2 uchar x 5 (general)", np.uint8, 5, rng.normal(0, 1, (2, 5)).tolist())):
            src = image(dtype, bands, 11)
            im = Image.new_from_array(src)
            report(name, lambda: im.recomb(m), src.nbytes, n * len(m) * 4, ref_chain("recomb:m=" + matrix_file(m), src))
            del im
        # clamp, remainder_const
        for dtype, bands in ((np.uint8, 3), (np.float32, 4)):
            src = image(dtype, bands, 13)
            im = Image.new_from_array(src)
            lo, hi = (16, 235) if dtype == np.uint8 else (0.1, 0.9)
            kind = "%s x %d" % (np.dtype(dtype).name, bands)
            report("clamp " + kind, lambda: im.clamp(lo, hi), src.nbytes, src.nbytes, ref_chain("clamp:min=%r,max=%r" % (lo, hi), src))
            report("remainder_const " + kind, lambda: im.remainder(7), src.nbytes, src.nbytes, ref_chain("remainder_const:c=7", src))
            del im
        # sum, bandrank
        vips = os.path.join(ROOT, "oracle", "_ref", "bin", "vips")
        arrays = [image(np.uint8, 3, 21 + i) for i in range(9)]
        images = [Image.new_from_array(a) for a in arrays]
        paths = []
        if WITH_REF and helpers.have_ref():
            for i, a in enumerate(arrays):
                paths.append(os.path.join(tmp, "n%d.v" % i))
                helpers.write_v(paths[-1], a, 22)

        def ref_cli(op, count):
            if not paths:
                return float("nan")
            best = float("inf")
            for _ in range(2):
                t0 = time.perf_counter()
                subprocess.run([vips, op, " ".join(paths[:count]), os.path.join(tmp, "out.v")], env=helpers.ref_cli_env(), check=True,
                               stdout=subprocess.DEVNULL)
                best = min(best, (time.perf_counter() - t0) * 1e3)
            return best

        for count in (3, 9):
            report("sum of %d uchar x 3" % count, lambda: Image.sum(images[:count]), count * n * 3, n * 3 * 4, ref_cli("sum", count))
            report("bandrank (median) of %d uchar x 3" % count, lambda: images[0].bandrank(images[1:count]), count * n * 3, n * 3,
                   ref_cli("bandrank", count))
    say("PERF-OK")
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
