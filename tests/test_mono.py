"""CPU: what holds the greyscale routes in place without a device -- the golden file is what the compiled reference
makes now, the colour step numbers of the public header did not move, and tests/test_mono_gpu.py itself passes
against libvipship_emul.so (the product's colour.hip on host fibers) under the mock HIP runtime."""
import os
import re
import sys

import numpy as np
import pytest

import libvips_amd
from tests import helpers
from tests.golden import make_mono_golden as mono
from tests.test_emul_gpu_suite import ENABLED, EMUL_SO, MOCK_SO

GOLD = np.load(os.path.join(helpers.GOLDEN, "mono.npz"))

# tests/test_mono_gpu.py: 203 cases, 8 of them drive the libvips module (they pass on host fibers as well where the
# module is built, but are not asked for here)
GPU_FILE_CASES = 203
MODULE_CASES = 8


def test_case_lists_and_golden_file_agree():
    names = [c[0] for c in mono.pair_cases()] + [c[0] for c in mono.TAG_CASES] + ["special|b-w", "special|grey16"] + \
        [c[0] for c in mono.THUMB_CASES]
    assert len(mono.pair_cases()) == 66 and len(set(names)) == len(names)
    assert sorted(GOLD.files) == sorted(names + [n + "#interp" for n in names])
    assert os.path.getsize(os.path.join(helpers.GOLDEN, "mono.npz")) < 1 << 20
    # 33 new pairs + the 25 there were = 58 of the reference's 64; the other 6 are the barred ones
    assert len(mono.PAIRS) + 25 + len(mono.BARRED) == 64
    for case in mono.THUMB_CASES:
        assert GOLD[case[0]].dtype == np.uint8 and int(GOLD[case[0] + "#interp"]) == mono.INTERP["b-w"], case[0]


@pytest.mark.skipif(not helpers.have_ref(), reason="oracle/_ref missing")
def test_golden_file_is_what_the_reference_makes_now():
    now = mono.generate()
    assert sorted(now) == sorted(GOLD.files)
    for name in now:
        want = GOLD[name]
        got = np.asarray(now[name])
        assert got.shape == want.shape and got.dtype == want.dtype, name
        assert np.array_equal(got.reshape(-1).view(np.uint8), want.reshape(-1).view(np.uint8)), name


def test_colour_step_numbers_of_the_header():
    """Tests and callers use the steps as numbers: the ten there were keep theirs, the new ones follow."""
    text = open(libvips_amd.HEADER_PATH).read()
    body = re.search(r"typedef enum \{([^}]*)\} VipsHipColourStep;", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip().split("=")[0].strip() for n in body.split(",") if n.strip()]
    assert names == ["VIPS_HIP_COLOUR_" + n for n in (
        "sRGB2scRGB", "scRGB2XYZ", "XYZ2Lab", "Lab2XYZ", "XYZ2scRGB", "scRGB2sRGB", "scRGB2sRGB16", "Lab2LabS",
        "LabS2Lab", "sRGB2scRGB16", "scRGB2BW", "scRGB2BW16", "BW2sRGB", "GREY162RGB16", "sRGB2RGB16", "RGB162sRGB",
        "LAST")]
    assert "VIPS_HIP_COLOUR_sRGB2scRGB = 0" in text
    for name in ("b-w", "grey16", "rgb16"):
        assert libvips_amd.INTERPRETATIONS[name] == mono.INTERP[name]


@pytest.mark.skipif(not ENABLED,
                    reason="a real GPU is present, or the reference / mock runtime / emulation cannot be built")
def test_mono_gpu_file_on_the_cpu():
    """tests/test_mono_gpu.py as a child process on host fibers: every route, the grey tables over every value, the
    region form, the launch counts and the thumbnails, against the same reference with the same assertions."""
    name = "mono:test_mono_gpu_file_on_the_cpu"
    env = dict(os.environ, LD_PRELOAD=MOCK_SO, VIPS_HIP_LIBRARY=EMUL_SO)
    cmd = [sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-p", "no:cacheprovider", "tests/test_mono_gpu.py"]
    helpers.Background.start(name, cmd, env=env, cwd=helpers.ROOT)
    rc, text = helpers.Background.wait(name)
    tail = text[-3000:]
    m = re.search(r"(\d+) passed", tail)
    assert rc == 0 and m and "failed" not in tail.splitlines()[-1], tail
    assert int(m.group(1)) >= GPU_FILE_CASES - MODULE_CASES, tail
