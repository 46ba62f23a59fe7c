"""TEST INFRASTRUCTURE for vips_labelregions / vips_countlines: the patterns tests/test_regions_host.py and
tests/test_regions_gpu.py share, a plain-Python restatement of both operations, and the compiled reference through its
command line on .v files (`vips labelregions in.v mask.v --segments` prints the count, `vips countlines in.v
horizontal` the number; the shim's ref_run asks every operation for an output called `out`, which labelregions does not
have).

The model: a raster scan that floods, 4-connected and on bytewise equality of whole pels, from every pel that has no
label yet; segments = regions + 1; countlines = rises / (extent across the direction x bands), in the reference's order
of divisions.  tests/test_regions_host.py pins it to the reference, so that a failure on the device points at a kernel."""
import os
import subprocess

import numpy as np

from tests import helpers

VIPS = os.path.join(helpers.ROOT, "oracle", "_ref", "bin", "vips")
MULTIBAND = 0
DIRECTIONS = ("horizontal", "vertical")


# ------------------------------------------------------------------ patterns: (h, w) arrays of small integers

def constant(w, h, value=1):
    return np.full((h, w), value, np.uint8)


def checkerboard(w, h):
    y, x = np.mgrid[0:h, 0:w]
    return ((x + y) & 1).astype(np.uint8)


def diagonal(w, h, period=2):
    """One-pel diagonal stripes of 1 every `period` pels on 0.  period 2: every pel is a region of its own (its diagonal
    neighbours are equal, its 4-neighbours are not); period 3: the ones are regions of one pel, the zeros two-pel
    staircases that hold together."""
    y, x = np.mgrid[0:h, 0:w]
    return ((x + y) % period == 0).astype(np.uint8)


def spiral(w, h):
    """A one-pel-wide spiral of 1 on 0, one pel of 0 between its turns, from the top-left corner inwards."""
    g = np.zeros((h, w), np.uint8)
    x = y = 0
    dx, dy = 1, 0
    g[0, 0] = 1
    while True:
        moved = False
        for _ in range(2):
            nx, ny, fx, fy = x + dx, y + dy, x + 2 * dx, y + 2 * dy
            if 0 <= nx < w and 0 <= ny < h and not g[ny, nx] and not (0 <= fx < w and 0 <= fy < h and g[fy, fx]):
                x, y = nx, ny
                g[y, x] = 1
                moved = True
                break
            dx, dy = -dy, dx
        if not moved:
            return g


def u_shape(w, h, left, right, top_left):
    """One U of 1 on 0: the right arm (column `right`) starts in row 0, the left one (column `left`) in row `top_left`;
    the last row joins them.  The region's raster-first pel is the top of the RIGHT arm."""
    g = np.zeros((h, w), np.uint8)
    g[top_left:, left] = 1
    g[:, right] = 1
    g[h - 1, left:right + 1] = 1
    return g


def many_us(w, h):
    """Us side by side, four columns each: left arm from row 2, a gap, right arm from row 0, a column of background."""
    g = np.zeros((h, w), np.uint8)
    for x0 in range(0, w - 2, 4):
        g[min(2, h - 1):, x0] = 1
        g[:, x0 + 2] = 1
        g[h - 1, x0:x0 + 3] = 1
    return g


def comb(w, h):
    """Teeth in every other column from row 0, joined on the last row only."""
    g = np.zeros((h, w), np.uint8)
    g[:, ::2] = 1
    g[h - 1, :] = 1
    return g


def noise(w, h, values, seed=7):
    return helpers.lcg_image(w, h, 1, np.uint8, seed)[:, :, 0] & (values - 1)


def spread(pattern, dtype, bands):
    """Every band holds the pattern's number, in `dtype`."""
    return np.repeat(pattern[:, :, None], bands, axis=2).astype(dtype)


def last_byte(pattern, dtype, bands):
    """Pels that differ in the last byte of the last band only: every other byte is 0x11."""
    h, w = pattern.shape
    pel = bands * np.dtype(dtype).itemsize
    raw = np.full((h, w, pel), 0x11, np.uint8)
    raw[:, :, pel - 1] = pattern
    return raw.view(dtype).reshape(h, w, bands)


def band_noise(w, h, bands, dtype, values, seed=7):
    """Independent noise of `values` values in every band."""
    return (helpers.lcg_image(w, h, bands, np.uint8, seed) & (values - 1)).astype(dtype)


# ------------------------------------------------------------------ the model

def _keys(array):
    """(h, w) integers, equal where the pels are bytewise equal."""
    a = np.ascontiguousarray(array)
    if a.ndim == 2:
        a = a[:, :, None]
    h, w, b = a.shape
    raw = a.view(np.uint8).reshape(h * w, b * a.dtype.itemsize)
    _, inverse = np.unique(raw, axis=0, return_inverse=True)
    return inverse.reshape(h, w)


def labelregions(array):
    """-> (mask (h, w) int32, segments)."""
    keys = _keys(array)
    h, w = keys.shape
    k = keys.tolist()
    mask = [[0] * w for _ in range(h)]
    segments = 1
    for y in range(h):
        for x in range(w):
            if mask[y][x]:
                continue
            key = k[y][x]
            mask[y][x] = segments
            stack = [(x, y)]
            while stack:
                cx, cy = stack.pop()
                for nx, ny in ((cx - 1, cy), (cx + 1, cy), (cx, cy - 1), (cx, cy + 1)):
                    if 0 <= nx < w and 0 <= ny < h and not mask[ny][nx] and k[ny][nx] == key:
                        mask[ny][nx] = segments
                        stack.append((nx, ny))
            segments += 1
    return np.array(mask, np.int32), segments


def rises(array, direction):
    """The number of rises: an element below 128 followed -- down its column for "horizontal", along its row for
    "vertical" -- by one at or above 128, every band counted."""
    a = np.asarray(array)
    if a.ndim == 2:
        a = a[:, :, None]
    white = a >= 128
    if direction == "horizontal":
        return int(np.count_nonzero(white[1:] & ~white[:-1]))
    return int(np.count_nonzero(white[:, 1:] & ~white[:, :-1]))


def countlines(array, direction):
    """vips_avg of the projection's uint sums (255 a rise) in double, then / 255.0 (countlines.c:98-118)."""
    a = np.asarray(array)
    if a.ndim == 2:
        a = a[:, :, None]
    h, w, b = a.shape
    vals = (w if direction == "horizontal" else h) * b
    return float(255 * rises(a, direction)) / float(vals) / 255.0


# ------------------------------------------------------------------ the compiled reference

def run_ref(args):
    r = subprocess.run([VIPS] + args, env=helpers.ref_cli_env(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if r.returncode != 0:
        raise RuntimeError((r.stderr.strip() or "vips %s failed" % args[0]).splitlines()[-1])
    return r.stdout


def _image(array):
    a = np.ascontiguousarray(array)
    return a[:, :, None] if a.ndim == 2 else a


def ref_labelregions(tmp_path, array):
    """-> (mask (h, w) int32, the mask's interpretation, segments) of the reference."""
    src, out = str(tmp_path / "in.v"), str(tmp_path / "mask.v")
    helpers.write_v(src, _image(array), MULTIBAND)
    segments = int(run_ref(["labelregions", src, out, "--segments"]).split()[0])
    mask, interpretation = helpers.read_v(out)
    assert mask.shape[2] == 1
    return mask[:, :, 0], interpretation, segments


def ref_countlines(tmp_path, array, direction):
    """-> the text the reference prints: the number with six decimals."""
    src = str(tmp_path / "in.v")
    helpers.write_v(src, _image(array), MULTIBAND)
    return run_ref(["countlines", src, direction]).strip()


def ref_rises(tmp_path, array, direction):
    """-> the reference's own projection of its own thresholded, convolved image, as the integers that vips_avg then
    adds: `vips relational_const`, `vips conv` with the (-1, 1) mask countlines.c:93 / :104 makes, `vips project`."""
    a = _image(array)
    src, t1, t2, c, r, m = [str(tmp_path / n) for n in ("in.v", "t1.v", "t2.v", "c.v", "r.v", "m.mat")]
    helpers.write_v(src, a, MULTIBAND)
    with open(m, "w") as f:
        f.write("1 2\n-1\n1\n" if direction == "horizontal" else "2 1\n-1 1\n")
    run_ref(["relational_const", src, t1, "moreeq", "128"])
    run_ref(["conv", t1, t2, m, "--precision", "integer"])
    run_ref(["project", t2, c, r])
    sums, _ = helpers.read_v(c if direction == "horizontal" else r)
    return sums.astype(np.uint64)
