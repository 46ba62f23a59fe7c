"""What the rot / flip / autorot tests share (tests/test_rot_gpu.py, tests/test_rot_host.py): the numpy statement of
every operation, the .v metadata trailer and the pel configurations.  numpy is a legitimate oracle for a permutation
of pels; tests/test_rot_gpu.py anchors these expressions to the compiled reference."""
import numpy as np

from tests import helpers

# VipsAngle, VipsDirection
ANGLES = {"d0": 0, "d90": 1, "d180": 2, "d270": 3}
DIRECTIONS = {"horizontal": 0, "vertical": 1}

# the five operations, as (height, width, bands) arrays
OPS = {
    "d90": lambda a: np.rot90(a, -1),
    "d180": lambda a: a[::-1, ::-1],
    "d270": lambda a: np.rot90(a, 1),
    "horizontal": lambda a: a[:, ::-1],
    "vertical": lambda a: a[::-1],
}
TRANSPOSING = ("d90", "d270")

# what vips_autorot makes of an orientation (conversion/autorot.c:119-177: the turn, then the horizontal flip)
ORIENT = {
    1: lambda a: a,
    2: lambda a: a[:, ::-1],
    3: lambda a: a[::-1, ::-1],
    4: lambda a: a[::-1, ::-1][:, ::-1],
    5: lambda a: np.rot90(a, -1)[:, ::-1],
    6: lambda a: np.rot90(a, -1),
    7: lambda a: np.rot90(a, 1)[:, ::-1],
    8: lambda a: np.rot90(a, 1),
}
# (angle, flip): vips_autorot's optional outputs
ORIENT_ANGLE_FLIP = {1: ("d0", False), 2: ("d0", True), 3: ("d180", False), 4: ("d180", True), 5: ("d90", True),
                     6: ("d90", False), 7: ("d270", True), 8: ("d270", False)}
SWAPS = (5, 6, 7, 8)

# (dtype, bands) for every pel size the tile kernel is compiled for, and the pel size
PELS = [(np.uint8, 1), (np.uint8, 2), (np.uint8, 3), (np.uint8, 4), (np.uint16, 1), (np.uint16, 2), (np.uint16, 3),
        (np.uint16, 4), (np.float32, 1), (np.float32, 2), (np.float32, 3), (np.float32, 4)]


def pel_size(dtype, bands):
    return np.dtype(dtype).itemsize * bands


def pel_id(case):
    return "%s_x%d" % (np.dtype(case[0]).name, case[1])


TRAILER = ('<?xml version="1.0"?>\n<root xmlns="http://www.vips.ecs.soton.ac.uk/vips/8.19.0">\n  <header>\n'
           '  </header>\n  <meta>\n    <field type="gint" name="orientation">%d</field>\n  </meta>\n</root>\n')


def write_oriented_v(path, array, orientation, interpretation=22):
    """helpers.write_v plus the metadata trailer of iofuncs/vips.c:560-622 with the one field (0: no trailer)."""
    helpers.write_v(path, array, interpretation)
    if orientation:
        with open(path, "ab") as f:
            f.write((TRAILER % orientation).encode())
    return path
