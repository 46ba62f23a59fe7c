"""GPU parity: every colour route kernel against the compiled reference on whole colour domains.

The kernels a user gets -- colour_lab_quad_kernel, colour_route_x4_kernel with a compiled-in route and with the
generic one -- need rows of whole quads, which the 37 x 29 goldens never have; the tiers behind them
(colour_lab_lds_kernel in both precisions, the static routes 1 and 2, other grids of the quad kernel) need an
environment variable or another libm.  Here each of them meets vips_colourspace of oracle/_ref (where that is
missing: the port, for the routes it has) on every uchar colour, on lattices / stratified floats / special values
for the sources that are not uchar-bounded, on the widths and heights round the quad kernel's block, and in region
form.  The rule (tests/colour_domains.py differing): same shape and dtype, bytes equal, signed zeros included;
elements that are NaN on both sides count as equal.  No tolerance, every pixel of every case.  Every case asserts
which kernel family ran, by the gate report.  Runs on the CPU too, on host fibers (tests/test_emul_gpu_suite.py)."""
import ctypes
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import libvips_amd
from libvips_amd import Image, _ffi
from tests import colour_domains as dom
from tests import helpers
from tests.helpers import INTERP, PortCC, Ref

pytestmark = pytest.mark.gpu

FORMATS = {np.dtype(np.uint8): 0, np.dtype(np.uint16): 2, np.dtype(np.int16): 3, np.dtype(np.float32): 6}
# include/vips_hip.h VipsHipColourStep
ROUTE_STEPS = {("srgb", "lab"): (0, 1, 2), ("srgb", "labs"): (0, 1, 2, 7), ("labs", "srgb"): (8, 3, 4, 5),
               ("lab", "srgb"): (3, 4, 5)}
OUT_DTYPE = {"lab": np.float32, "labs": np.int16, "srgb": np.uint8}
QUAD, LDS, STATIC, X4, ONE = "colour_lab_quad", "colour_lab_lds", "colour_route_x4_static", "colour_route_x4", "colour_route"
FAMILIES = (QUAD, LDS, STATIC, X4, ONE)


@pytest.fixture(scope="module", autouse=True)
def _init():
    libvips_amd.init(0)


def reference(src, a, b):
    if helpers.have_ref():
        return Ref.run("colourspace", src, "space=" + b, INTERP[a])
    if (a, b) not in PortCC._ROUTES:
        pytest.skip("oracle/_ref missing and the port has no %s -> %s" % (a, b))
    return PortCC.colourspace(src, b, a)


class gated(object):
    """with gated() as g: ...; g.report: {gate name: (launches, ms)} of what ran inside."""

    def __enter__(self):
        _ffi.lib.vips_hip_gate_reset()
        _ffi.lib.vips_hip_gate_enable(1)
        self.report = None
        return self

    def __exit__(self, *exc):
        try:
            if exc[0] is None:
                self.report = libvips_amd.gate_report()
        finally:
            _ffi.lib.vips_hip_gate_enable(0)
            _ffi.lib.vips_hip_gate_reset()
        return False


def hip_colourspace(src, a, b):
    with gated() as g:
        got = Image.new_from_array(src, interpretation=a).colourspace(b).numpy()
    return got, g.report


def whole_image_gate(a, b, fmt=None):
    """The gate of a 3-band image of whole quads on its way from a to b."""
    if a == "srgb" and b in ("lab", "labs"):
        return QUAD
    if (a, b) in (("labs", "srgb"), ("lab", "srgb")):
        return STATIC
    if b in ("b-w", "grey16"):
        return "colour_grey_x4"
    if (a, b) in (("srgb", "rgb16"), ("rgb16", "srgb")):
        return "colour_mono"  # (a shift cast on its own)
    return X4


def check(src, a, b, gate, what=None):
    what = what or "%s %s -> %s %s" % (src.dtype.name, a, b, src.shape)
    want = reference(src, a, b)
    got, report = hip_colourspace(src, a, b)
    assert sorted(report) == sorted(gate if isinstance(gate, (list, tuple)) else [gate]), (what, report)
    dom.assert_same(got, want, what, src)
    return want


# ---- a. every colour

def cube_source(fmt):
    return dom.cube() if fmt == "u8" else dom.cube().astype(np.float32)


CUBE_CASES = [(fmt, b) for fmt in ("u8", "f32") for b in ("scrgb", "xyz", "lab", "labs", "b-w", "grey16")] + [("u8", "rgb16")]


@pytest.mark.parametrize("fmt,space", CUBE_CASES, ids=["%s-%s" % c for c in CUBE_CASES])
def test_every_colour(fmt, space):
    """All 2^24 uchar colours, as uchar and as the same values in float (the fast kernels clip a float to uchar
    first, so this is their whole domain)."""
    check(cube_source(fmt), "srgb", space, whole_image_gate("srgb", space))


@pytest.mark.parametrize("space", ["labs", "lab", "xyz", "scrgb"])
def test_every_colour_back(space):
    """The reference's own image of the cube in each space, back to sRGB: the reference's bytes, which are the cube."""
    cube = dom.cube()
    there = reference(cube, "srgb", space)
    back = check(there, space, "srgb", whole_image_gate(space, "srgb"))
    if helpers.have_ref():
        dom.assert_same(back, cube, "the reference's srgb -> %s -> srgb" % space)


# ---- b. the float -> uchar clip in front of the fast kernels

@pytest.mark.parametrize("space", ["lab", "labs", "xyz"])
def test_float_clip(space):
    check(dom.float_clip(), "srgb", space, whole_image_gate("srgb", space))


# ---- c. the tiers

TIERS = {
    "no-cbrt-quad": ({"VIPS_HIP_NO_CBRT_QUAD": "1"}, LDS,
                     ("cbrt_quad_tables: this host's cbrtf does not fit the scheme (check 1)",
                      "cbrt_exact_tables: the single-precision form")),
    "no-cbrt-quad-f64": ({"VIPS_HIP_NO_CBRT_QUAD": "1", "VIPS_HIP_CBRT_F64": "1"}, LDS,
                         ("cbrt_quad_tables: this host's cbrtf does not fit the scheme (check 1)",
                          "cbrt_exact_tables: the double form")),
    "no-lab-lds": ({"VIPS_HIP_NO_LAB_LDS": "1"}, STATIC, ()),
    "quad-grid-1": ({"VIPS_HIP_LAB_QUAD_GRID": "1"}, QUAD, ("cbrt_quad_tables: every pair checked",)),
    "quad-grid-7": ({"VIPS_HIP_LAB_QUAD_GRID": "7"}, QUAD, ("cbrt_quad_tables: every pair checked",)),
}
TIER_ENV = ("VIPS_HIP_NO_CBRT_QUAD", "VIPS_HIP_CBRT_F64", "VIPS_HIP_NO_LAB_LDS", "VIPS_HIP_LAB_QUAD_GRID",
            "VIPS_HIP_DEBUG_CBRT")
TIER_OUTPUTS = [(fmt, space) for space in ("lab", "labs") for fmt in ("u8", "f32")]
TIER_TIMEOUT = 600

TIER_CHILD = r'''
import sys
sys.path.insert(0, %(root)r)
import json
import numpy as np
import libvips_amd
from libvips_amd import Image
from tests import colour_domains as dom

libvips_amd.init(0)
lib = libvips_amd.lib
lib.vips_hip_set_exact_float(1)
reports = {}
for space in ("lab", "labs"):
    for fmt in ("u8", "f32"):
        src = dom.cube() if fmt == "u8" else dom.cube().astype(np.float32)
        lib.vips_hip_gate_reset()
        lib.vips_hip_gate_enable(1)
        out = Image.new_from_array(src, interpretation="srgb").colourspace(space).numpy()
        reports["%%s-%%s" %% (fmt, space)] = libvips_amd.gate_report()
        lib.vips_hip_gate_enable(0)
        np.save(%(out)r + "/%%s-%%s.npy" %% (fmt, space), out)
        del out, src
with open(%(out)r + "/reports.json", "w") as f:
    json.dump(reports, f)
print("CHILD-OK")
'''

# the output of the first child that ended by a signal or its time limit: nothing more is started after it
_tier_stop = []


@pytest.mark.parametrize("tier", list(TIERS))
def test_tier(tier, tmp_path):
    """The kernels behind the default one, each in a fresh process (the choice of table is made once per process and
    device): the whole cube to Lab and LabS from both source formats; the child's stderr names the cube-root form."""
    if _tier_stop:
        pytest.fail("not started: an earlier tier child ended abnormally\n" + _tier_stop[0])
    env_add, gate, messages = TIERS[tier]
    env = {k: v for k, v in os.environ.items() if k not in TIER_ENV}
    env.update(env_add, VIPS_HIP_DEBUG_CBRT="1")
    out = str(tmp_path / "out")
    os.mkdir(out)
    script = str(tmp_path / "child.py")
    with open(script, "w") as f:
        f.write(TIER_CHILD % {"root": helpers.ROOT, "out": out})
    try:
        try:
            proc = subprocess.run([sys.executable, script], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                                  env=env, cwd=helpers.ROOT, timeout=TIER_TIMEOUT)
        except subprocess.TimeoutExpired as e:
            _tier_stop.append("%s: no end after %d s\n%s" % (tier, TIER_TIMEOUT, str(e.stderr)[-2000:]))
            pytest.fail(_tier_stop[0])
        text = "%s: exit status %d\n%s\n%s" % (tier, proc.returncode, proc.stdout[-1500:], proc.stderr[-2500:])
        if proc.returncode < 0 or proc.returncode in (124, 134, 137, 139):
            _tier_stop.append(text)
        assert proc.returncode == 0 and "CHILD-OK" in proc.stdout, text
        cbrt_lines = [line for line in proc.stderr.splitlines() if line.startswith("cbrt_")]
        assert cbrt_lines == list(messages), text
        import json

        reports = json.load(open(os.path.join(out, "reports.json")))
        for fmt, space in TIER_OUTPUTS:
            name = "%s-%s" % (fmt, space)
            assert sorted(reports[name]) == [gate], (tier, name, reports[name])
            got = np.load(os.path.join(out, name + ".npy"), mmap_mode="r")
            src = cube_source(fmt)
            dom.assert_same(got, reference(src, "srgb", space), "%s %s" % (tier, name), src)
            del got
    finally:
        shutil.rmtree(out, ignore_errors=True)


# ---- d. wide domains for the routes that are not uchar-bounded

@pytest.mark.parametrize("name,target", dom.WIDE_CASES, ids=["%s-%s" % c for c in dom.WIDE_CASES])
def test_wide_domain(name, target):
    src, space = dom.wide_source(name)
    check(src, space, target, whole_image_gate(space, target), "%s -> %s" % (name, target))


# ---- e. layout

LAYOUT_ROUTES = [("srgb", "u8", "lab"), ("srgb", "f32", "lab"), ("srgb", "u8", "labs"), ("srgb", "f32", "labs"),
                 ("labs", "s16", "srgb"), ("lab", "f32", "srgb")]
ROUTE_IDS = ["%s-%s-%s" % r for r in LAYOUT_ROUTES]


@pytest.mark.parametrize("width", [4, 4092, 4096, 4100, 8196])
@pytest.mark.parametrize("route", LAYOUT_ROUTES, ids=ROUTE_IDS)
def test_widths_and_heights(route, width):
    """The quad kernel's block covers 4096 pixels of a row: one lane, one lane short of a block, a block, one lane
    over, two blocks and a lane; heights of 1, 2, and either side of the 256 blocks that share the rows out."""
    a, fmt, b = route
    for height in (1, 2, 255, 257, 1031):
        src = dom.layout_input(a, fmt, width, height, 3, 700 + height)
        check(src, a, b, whole_image_gate(a, b))


@pytest.mark.parametrize("width", [3, 5, 4095, 4097])
@pytest.mark.parametrize("route", LAYOUT_ROUTES, ids=ROUTE_IDS)
def test_widths_of_no_whole_quads(route, width):
    a, fmt, b = route
    check(dom.layout_input(a, fmt, width, 19, 3, 720 + width), a, b, ONE)


@pytest.mark.parametrize("bands", [4, 5])
@pytest.mark.parametrize("route", LAYOUT_ROUTES, ids=ROUTE_IDS)
def test_extra_bands(route, bands):
    """4 bands and 3 + 2: step by step through the one-pixel-per-lane kernel, on a width the fast kernels would take;
    the extra bands are the reference's too (check compares every band).  A float sRGB image is cast to uchar as a
    whole first, as the reference does it: its extra bands are clipped with the colour bands (alpha 159.2 -> 159)."""
    a, fmt, b = route
    src = dom.layout_input(a, fmt, 4096, 9, bands, 730 + bands)
    want = check(src, a, b, ["cast", ONE] if (a, fmt) == ("srgb", "f32") else ONE)
    assert want.shape[2] == bands


# (name, input image width, window of the input image that is uploaded: x0 y0 w h, output rectangle: left top w h,
#  is it a case for the 4-pixels-per-lane kernels?)
REGION_CASES = [
    ("inside-aligned", 128, (0, 0, 128, 40), (8, 3, 64, 30), True),
    ("inside-aligned-window", 128, (16, 2, 96, 36), (24, 5, 80, 20), True),
    ("left-breaks-pointer", 128, (0, 0, 128, 40), (9, 3, 64, 30), False),
    ("left-breaks-pointer-by-2", 128, (4, 0, 120, 40), (6, 0, 64, 40), False),
    ("stride-not-of-quads", 128, (0, 0, 101, 40), (8, 3, 64, 30), False),
    ("stride-not-of-quads-whole-rows", 128, (3, 1, 102, 30), (3, 1, 100, 30), False),
    ("width-not-of-quads", 128, (0, 0, 128, 40), (8, 3, 63, 30), False),
]


@pytest.mark.parametrize("case", REGION_CASES, ids=[c[0] for c in REGION_CASES])
@pytest.mark.parametrize("route", LAYOUT_ROUTES, ids=ROUTE_IDS)
def test_region_form(route, case):
    """vips_hip_colour_route_gen: an output rectangle inside a larger input region.  The input pointer the kernel
    gets is the region's plus the rectangle's offset, its stride the region's: each can take the image off the
    4-pixels-per-lane kernels, and the report must say so."""
    a, fmt, b = route
    _, full_w, (x0, y0, ww, wh), (left, top, w, h), fast = case
    full_h = 40
    src = dom.layout_input(a, fmt, full_w, full_h, 3, 740)
    want = reference(src, a, b)
    win = Image.new_from_array(np.ascontiguousarray(src[y0:y0 + wh, x0:x0 + ww]))
    rin = win.region()
    rin.left, rin.top, rin.im_width, rin.im_height = x0, y0, full_w, full_h
    out = Image.new_from_array(np.zeros((h, w, 3), OUT_DTYPE[b]))
    rout = out.region()
    rout.left, rout.top, rout.im_width, rout.im_height = left, top, full_w, full_h
    assert rin.format == FORMATS[src.dtype] and rin.stride == ww * 3 * src.dtype.itemsize
    steps = (ctypes.c_int * len(ROUTE_STEPS[(a, b)]))(*ROUTE_STEPS[(a, b)])
    with gated() as g:
        _ffi.check(_ffi.lib.vips_hip_colour_route_gen(steps, len(steps), ctypes.c_double(1.0), ctypes.byref(rin),
                                                      ctypes.byref(rout)))
        got = out.numpy()
    assert sorted(g.report) == [whole_image_gate(a, b) if fast else ONE], (case[0], g.report)
    dom.assert_same(got, np.ascontiguousarray(want[top:top + h, left:left + w]), "%s %s" % (route, case[0]))
