"""CPU: tests/test_rot_gpu.py itself, run against libvipship_emul.so under the mock HIP runtime: rot.hip's kernels on
host fibers (tests/emul/rot_emul.cpp), the same oracle, the same assertions, the gate names included.  Started by the
launcher of tests/test_emul_gpu_suite.py; the cases that need the libvips module skip themselves there."""
import pytest

from tests import test_emul_gpu_suite as suite

pytestmark = pytest.mark.skipif(not suite.ENABLED,
                                reason="a real GPU is present, or the reference / mock runtime / emulation cannot be built")

NAME = "test_rot_file_on_the_cpu"
# test -> (files, -k deselections, at least this many cases must pass): 96 kernel cases, 8 double, 12 behind the
# switch, 8 many-tile, 1 orientation, 2 anchors, 5 region views, 32 + 1 + 4 thumbnails, the .v round trip; the two
# JPEG cases need Pillow and a reference with libjpeg; 6 + 5 second turns of the capped grids
suite.JOBS[NAME] = (["tests/test_rot_gpu.py"], [], 181)


def test_rot_file_on_the_cpu():
    """tests/test_rot_gpu.py, all of it but the module cases."""
    suite._run(NAME)
