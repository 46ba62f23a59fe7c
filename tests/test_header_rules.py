"""CPU: the header rules the op families share (libvips_amd/csrc/header_rules.cpp) against the compiled reference, on
the headers where the one guess_interpretation answers differently from the two copies it replaced: tags vips_hip.h has
no name for on images they cannot be true of, HISTOGRAM on an image that is no histogram, and the MATRIX default of
one-band char.  A .v file carries each header to both sides: `vips colourspace` / `vips hist_equal` / `vips maplut` of
oracle/_ref, and the product on host fibers under the mock runtime (one child process for all cases)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import helpers
from tests.test_emul_resize_sharpen import EMUL_SO, _build_emul
from tests.test_host_glue_mock import MOCK_SO, _build_mock, _gpu_present

pytestmark = pytest.mark.skipif(_gpu_present() or not helpers.have_ref() or not _build_mock() or not _build_emul(),
                                reason="a real GPU is present, or the reference / mock runtime / emulation cannot be built")

VIPS = os.path.join(helpers.ROOT, "oracle", "_ref", "bin", "vips")

# name -> (shape, dtype, the tag in the header, the operation, its argument).  Every image is more than one pel wide
# and high; the tags by number are VipsInterpretation's (include/vips/image.h:94-118).
CASES = {
    # vips_hip_colourspace: the copy it had kept these tags, and answered "no known route from 'unknown'"
    "histogram_3band": ((2, 3, 3), np.uint8, 10, "colourspace", "lab"),   # no histogram: sRGB by the default
    "rgb_1band": ((2, 3, 1), np.uint8, 17, "colourspace", "srgb"),        # too few bands for RGB: B_W
    "cmyk_3band": ((2, 3, 3), np.uint8, 15, "colourspace", "lab"),        # too few bands for CMYK: sRGB
    "yxy_uchar": ((2, 3, 3), np.uint8, 23, "colourspace", "lab"),         # YXY needs float: sRGB
    "labq_uncoded": ((2, 3, 3), np.uint8, 16, "colourspace", "lab"),      # LABQ needs the coding: sRGB
    "fourier_float": ((2, 3, 3), np.float32, 24, "colourspace", "lab"),   # FOURIER needs complex: sRGB
    "oklab_ushort": ((2, 3, 3), np.uint16, 30, "colourspace", "srgb"),    # OKLAB needs float: RGB16
    # (the .v loader reads ERROR as MULTIBAND: the product's image is made with the tag, from the file's pixels)
    "error_tag": ((2, 3, 3), np.uint8, -1, "colourspace", "lab"),
    # vips_hip_maplut (under vips_hip_hist_equal): the copy it had kept these tags on the result
    "hist_equal_rgb_1band": ((2, 3, 1), np.uint8, 17, "hist_equal", None),
    "hist_equal_yxy_1band": ((2, 3, 1), np.uint8, 23, "hist_equal", None),
    "hist_equal_labq_1band": ((2, 3, 1), np.uint8, 16, "hist_equal", None),
    # ... and called a one-band char result MULTIBAND, which the reference calls MATRIX (27)
    "maplut_char_table": ((2, 3, 1), np.uint8, 0, "maplut", "char"),
}

CHILD = r'''
import json, sys
sys.path.insert(0, %(root)r)
import libvips_amd
from libvips_amd import Image
from tests import helpers
libvips_amd.init(0)
errors = {}
for name, (op, arg, src, dst, lut, tag) in sorted(json.load(open(sys.argv[1])).items()):
    try:
        im = Image.new_from_file(src) if tag >= 0 else Image.new_from_array(helpers.read_v(src)[0], interpretation=tag)
        if op == "colourspace":
            out = im.colourspace(arg)
        elif op == "hist_equal":
            out = im.hist_equal()
        else:
            out = im.maplut(Image.new_from_file(lut))
        out.write_to_file(dst)
    except Exception as e:
        errors[name] = str(e)
json.dump(errors, open(sys.argv[2], "w"))
'''


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("header_rules")
    rng = np.random.RandomState(7)
    lut = str(tmp / "lut.v")
    helpers.write_v(lut, (np.arange(256) - 128).astype(np.int8).reshape(1, 256, 1), 10)
    jobs, want = {}, {}
    for name, (shape, dtype, tag, op, arg) in CASES.items():
        src, ref, dst = (str(tmp / (name + suffix)) for suffix in (".v", "_ref.v", "_hip.v"))
        helpers.write_v(src, (rng.rand(*shape) * 250).astype(dtype), tag)
        cmd = [VIPS, op, src, ref] + ([lut] if op == "maplut" else [arg] if arg else [])
        r = subprocess.run(cmd, env=helpers.ref_cli_env(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert r.returncode == 0, (name, r.stderr)
        want[name] = helpers.read_v(ref)
        jobs[name] = (op, arg, src, dst, lut, tag)
    script, spec, errors = str(tmp / "child.py"), str(tmp / "jobs.json"), str(tmp / "errors.json")
    open(script, "w").write(CHILD % {"root": helpers.ROOT})
    json.dump(jobs, open(spec, "w"))
    r = subprocess.run([sys.executable, script, spec, errors], env=dict(os.environ, LD_PRELOAD=MOCK_SO, VIPS_HIP_LIBRARY=EMUL_SO),
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=helpers.ROOT)
    assert r.returncode == 0, r.stdout[-3000:]
    return want, {name: job[3] for name, job in jobs.items()}, json.load(open(errors))


@pytest.mark.parametrize("name", sorted(CASES))
def test_guess_interpretation_is_the_references(results, name):
    want, outputs, errors = results
    assert name not in errors, errors[name]
    got_pixels, got_tag = helpers.read_v(outputs[name])
    want_pixels, want_tag = want[name]
    assert got_tag == want_tag
    assert got_pixels.dtype == want_pixels.dtype and got_pixels.shape == want_pixels.shape
    assert np.array_equal(got_pixels.view(np.uint8), want_pixels.view(np.uint8))
