"""Generate tests/golden/mono.npz from the COMPILED REFERENCE (oracle/_ref): the greyscale and 16-bit RGB routes
of vips_colourspace and the thumbnails of images with fewer than three bands.

Run where oracle/_ref exists: `python tests/golden/make_mono_golden.py`.  Inputs are made again from seeds
(tests.helpers.lcg_image), so only the reference's outputs (and the interpretation it tags them with) are stored.
The case lists below are what tests/test_mono_gpu.py and tests/test_mono.py walk.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import helpers  # noqa: E402

INTERP = {"multiband": 0, "b-w": 1, "xyz": 12, "lab": 13, "labs": 21, "srgb": 22, "rgb16": 25, "grey16": 26,
          "scrgb": 28}
SPACES = ["b-w", "grey16", "rgb16", "srgb", "scrgb", "xyz", "lab", "labs"]
NEW = ("b-w", "grey16", "rgb16")
# the pairs of the reference's table (colourspace.c:223-497) this library leaves out
BARRED = [(a, b) for a in ("b-w", "grey16") for b in ("xyz", "lab", "labs")]
# what this pull request adds: every pair with a new space on either side, but the barred ones
PAIRS = [(a, b) for a in SPACES for b in SPACES if (a in NEW or b in NEW) and (a, b) not in BARRED]
assert len(PAIRS) == 33

COLOUR_BANDS = {"b-w": 1, "grey16": 1}


def space_input(space, width, height, extra, seed):
    """An image in `space`'s own format with `extra` bands behind its colour bands."""
    bands = COLOUR_BANDS.get(space, 3) + extra
    a = helpers.lcg_image(width, height, bands, np.uint8, seed)
    if space in ("b-w", "srgb"):
        return a
    if space in ("grey16", "rgb16"):
        return helpers.lcg_image(width, height, bands, np.uint16, seed)
    if space == "scrgb":
        return (a.astype(np.float32) / 200.0 - 0.1).astype(np.float32)
    if space == "xyz":
        return (a.astype(np.float32) / 2.3).astype(np.float32)
    if space == "lab":
        f = a.astype(np.float32)
        f[:, :, 0] = f[:, :, 0] / 2.55
        f[:, :, 1:3] -= 128
        return f
    if space == "labs":
        s = helpers.lcg_image(width, height, bands, np.int16, seed)
        s[:, :, 0] = np.abs(s[:, :, 0])
        return s
    raise ValueError(space)


def pair_cases():
    """(name, source space, target space, extra bands, seed) at 37 x 29"""
    out = []
    for i, (a, b) in enumerate(PAIRS):
        for extra in (0, 1):
            out.append(("pair|%s|%s|%d" % (a, b, extra), a, b, extra, 400 + i))
    return out


# a ushort image whose tag is not the 16-bit one decodes the 8-bit way, clipping (sRGB2scRGB.c:115-123)
TAG_CASES = [
    ("tag|ushort3-srgb|b-w", 3, "srgb", "b-w"),
    ("tag|ushort3-srgb|grey16", 3, "srgb", "grey16"),
    ("tag|ushort3-srgb|rgb16", 3, "srgb", "rgb16"),
    ("tag|ushort1-b-w|grey16", 1, "b-w", "grey16"),
    ("tag|ushort1-b-w|srgb", 1, "b-w", "srgb"),
]


def tag_input(bands):
    a = helpers.lcg_image(61, 43, bands, np.uint16, 471)
    a[::2] >>= 8  # (half the rows inside 0 .. 255, where the clipping cast keeps them apart)
    return a


def special_input():
    nan = np.nan
    return np.array([[[nan, 0.5, 0.5], [0.5, nan, 0.5], [0.5, 0.5, nan], [-0.25, -1.0, -0.5], [2.0, 1.5, 3.0],
                      [1e30, 0.0, 0.0], [0.0, -1e30, 0.0], [1e30, -1e30, 0.5], [0.999999, 0.999999, 0.999999],
                      [1e-40, 1e-39, 1e-41], [0.0, 1.0, 0.0], [1.0, 1.0, 1.0], [np.inf, 0.0, 0.0],
                      [np.inf, -np.inf, 0.0], [0.2, 0.4, 0.6], [0.0031308, 0.0031308, 0.0031308]]], np.float32)


# (name, source: (width, height, bands, dtype, interpretation), thumbnail_image arguments)
THUMB_CASES = [
    ("thumb|uchar-ga", (300, 200, 2, np.uint8, "b-w"), "width=60"),
    ("thumb|ushort-g", (300, 200, 1, np.uint16, "grey16"), "width=60"),
    ("thumb|ushort-ga", (300, 200, 2, np.uint16, "grey16"), "width=60"),
    ("thumb|float-g", (300, 200, 1, np.float32, "b-w"), "width=60"),
    ("thumb|uchar-g|linear", (300, 200, 1, np.uint8, "b-w"), "width=60,linear=true"),
    ("thumb|uchar-ga|linear", (300, 200, 2, np.uint8, "b-w"), "width=60,linear=true"),
    ("thumb|ushort-g|linear", (300, 200, 1, np.uint16, "grey16"), "width=60,linear=true"),
    ("thumb|uchar-ga|crop", (300, 200, 2, np.uint8, "b-w"), "width=60,height=60,crop=centre"),
    ("thumb|uchar-ga|force", (300, 200, 2, np.uint8, "b-w"), "width=60,size=force"),
    ("thumb|uchar-ga|down-small", (40, 30, 2, np.uint8, "b-w"), "width=60,size=down"),
]


def thumb_input(case):
    w, h, bands, dtype, _ = case[1]
    return helpers.lcg_image(w, h, bands, dtype, 480)


def generate():
    """Every stored case from the reference as it is now: {name: pixels, name + "#interp": tag}."""
    out = {}

    def keep(name, result):
        pixels, interp = result
        out[name] = pixels
        out[name + "#interp"] = np.int32(interp)

    for name, a, b, extra, seed in pair_cases():
        keep(name, helpers.Ref.run_interp("colourspace", space_input(a, 37, 29, extra, seed), "space=" + b, INTERP[a]))
    for name, bands, tag, space in TAG_CASES:
        keep(name, helpers.Ref.run_interp("colourspace", tag_input(bands), "space=" + space, INTERP[tag]))
    for space in ("b-w", "grey16"):
        keep("special|" + space, helpers.Ref.run_interp("colourspace", special_input(), "space=" + space, INTERP["scrgb"]))
    for case in THUMB_CASES:
        keep(case[0], helpers.Ref.run_interp("thumbnail_image", thumb_input(case), case[2], INTERP[case[1][4]]))
    return out


def main():
    out = generate()
    path = os.path.join(helpers.GOLDEN, "mono.npz")
    np.savez_compressed(path, **out)
    print("mono.npz: %d arrays, %d bytes" % (len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
