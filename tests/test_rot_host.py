"""CPU: the host side of rot / flip / autorot -- the orientation in a .v file's metadata trailer, the swapped box of
the shrink-on-load factor, and the error behaviour of the new entry points.  No device needed."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from libvips_amd import _ffi
from tests import helpers
from tests.rot_cases import TRAILER, write_oriented_v

lib = _ffi.lib
VIPS_CLI = os.path.join(helpers.ROOT, "oracle", "_ref", "bin", "vips")


def read_orientation(path):
    value = ctypes.c_int(-1)
    assert lib.vips_hip_vfile_read_orientation(os.fsencode(path), ctypes.byref(value)) == 0, _ffi.error_buffer()
    return value.value


@pytest.fixture(scope="module")
def pixels():
    return helpers.lcg_image(23, 17, 3, np.uint8, 5)


def test_trailer_orientations(tmp_path, pixels):
    for orientation in range(1, 9):
        path = write_oriented_v(str(tmp_path / "o.v"), pixels, orientation)
        assert read_orientation(path) == orientation
    # a value that is no orientation is none
    for bad in (0, 9, 77):
        helpers.write_v(str(tmp_path / "bad.v"), pixels)
        with open(str(tmp_path / "bad.v"), "ab") as f:
            f.write((TRAILER % bad).encode())
        assert read_orientation(str(tmp_path / "bad.v")) == 0


def test_no_trailer_and_a_trailer_without_the_field(tmp_path, pixels):
    path = str(tmp_path / "plain.v")
    helpers.write_v(path, pixels)
    assert read_orientation(path) == 0
    other = TRAILER.replace('name="orientation"', 'name="page-height"') % 6
    with open(path, "ab") as f:
        f.write(other.encode())
    assert read_orientation(path) == 0
    # the field outside <meta> is not the image's metadata
    helpers.write_v(path, pixels)
    with open(path, "ab") as f:
        f.write(b'<?xml version="1.0"?>\n<root>\n  <header>\n    <field type="gint" name="orientation">6</field>\n'
                b'  </header>\n  <meta>\n  </meta>\n</root>\n')
    assert read_orientation(path) == 0


def test_truncated_trailer(tmp_path, pixels):
    """Cut anywhere, a trailer gives no orientation (the reference's XML parser refuses a document that does not
    end) and no crash."""
    whole = (TRAILER % 6).encode()
    path = str(tmp_path / "cut.v")
    for keep in range(0, len(whole) - len(b"</meta>\n</root>\n")):
        helpers.write_v(path, pixels)
        with open(path, "ab") as f:
            f.write(whole[:keep])
        assert read_orientation(path) == 0, keep


@pytest.mark.skipif(not os.path.exists(VIPS_CLI), reason="oracle/_ref not built")
def test_trailer_the_reference_wrote(tmp_path, pixels):
    for orientation in (6, 3):
        ours = write_oriented_v(str(tmp_path / "ours.v"), pixels, orientation)
        theirs = str(tmp_path / "theirs.v")
        subprocess.run([VIPS_CLI, "copy", ours, theirs], check=True, env=helpers.ref_cli_env())
        assert b'name="orientation"' in open(theirs, "rb").read()
        assert read_orientation(theirs) == orientation
        got, _ = helpers.read_v(theirs)
        assert np.array_equal(got, pixels)


def test_read_orientation_errors(tmp_path):
    value = ctypes.c_int()
    lib.vips_hip_error_clear()
    assert lib.vips_hip_vfile_read_orientation(None, ctypes.byref(value)) != 0
    assert "null argument" in _ffi.error_buffer()
    lib.vips_hip_error_clear()
    assert lib.vips_hip_vfile_read_orientation(os.fsencode(str(tmp_path / "missing.v")), ctypes.byref(value)) != 0
    assert "unable to open" in _ffi.error_buffer()
    lib.vips_hip_error_clear()


def test_jpegshrink_with_the_box_swapped():
    """thumbnail.c:418-420: an image that will be turned by a quarter is shrunk for the swapped box."""
    new, old = lib.vips_hip_thumbnail_find_jpegshrink_rotate, lib.vips_hip_thumbnail_find_jpegshrink
    factors = set()
    for w, h in ((4000, 3000), (3000, 4000), (1024, 768), (640, 4800), (300, 200), (17, 9)):
        for W, H in ((64, 64), (100, 80), (80, 100), (256, 32), (32, 256), (1000, 1000), (50, 0)):
            for size in range(4):
                for linear in (0, 1):
                    for crop in (0, 1):
                        box_h = H or W
                        assert new(w, h, W, H, size, linear, crop, 1) == old(w, h, box_h, W, size, linear, crop)
                        assert new(w, h, W, H, size, linear, crop, 0) == old(w, h, W, H, size, linear, crop)
                        factors.add((new(w, h, W, H, size, linear, crop, 1), new(w, h, W, H, size, linear, crop, 0)))
    # the grid is worth something: every factor turns up, and the swap changes it somewhere
    assert {f for pair in factors for f in pair} == {1, 2, 4, 8} and any(a != b for a, b in factors)


def test_null_and_zero_arguments_are_errors():
    out = ctypes.c_void_p()
    region = _ffi.Region()
    calls = [
        ("vips_hip_rot", (None, ctypes.byref(out), 1), "null argument"),
        ("vips_hip_rot", (None, None, 0), "null argument"),
        ("vips_hip_rot", (None, ctypes.byref(out), 4), "bad angle"),
        ("vips_hip_flip", (None, ctypes.byref(out), 0), "null argument"),
        ("vips_hip_flip", (None, ctypes.byref(out), 2), "bad direction"),
        ("vips_hip_autorot", (None, ctypes.byref(out), None, None), "null argument"),
        ("vips_hip_rot_gen", (9, ctypes.byref(region), ctypes.byref(region)), "bad angle"),
        ("vips_hip_flip_gen", (-1, ctypes.byref(region), ctypes.byref(region)), "bad direction"),
        ("vips_hip_rot_gen", (1, None, None), ""),
        ("vips_hip_flip_gen", (0, None, None), ""),
        ("vips_hip_image_set_orientation", (None, 6), "null argument"),
        ("vips_hip_thumbnail_image_rotate", (None, ctypes.byref(out), 10, 10, 0, 0, 0, 0), "null argument"),
        ("vips_hip_thumbnail_rotate", (None, ctypes.byref(out), 10, 10, 0, 0, 0, 0), "null argument"),
        ("vips_hip_thumbnail_rotate", (b"x.v", ctypes.byref(out), 0, 0, 0, 0, 0, 0), "width not set"),
        ("vips_hip_thumbnail_batch_rotate", (None, 0, None, None, 10, 10, 0, 0, 0, 0, 1), "null argument"),
        ("vips_hip_thumbnail_find_jpegshrink_rotate", (0, 0, 0, 0, 0, 0, 0, 0), "bad dimensions"),
    ]
    for name, args, words in calls:
        lib.vips_hip_error_clear()
        assert getattr(lib, name)(*args) != 0, name
        message = _ffi.error_buffer()
        assert message.strip() and words in message, (name, message)
    lib.vips_hip_error_clear()
    assert lib.vips_hip_image_get_orientation(None) == 0
    assert lib.vips_hip_rot_tile_side(0) == 0 and lib.vips_hip_rot_tile_side(5) == 0
    assert [lib.vips_hip_rot_tile_side(p) for p in (1, 2, 3, 4, 6, 8, 12, 16)] == [64] * 6 + [32] * 2
