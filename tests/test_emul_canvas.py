"""CPU: tests/test_canvas_gpu.py itself, run against libvipship_emul.so under the mock HIP runtime: canvas.hip's kernels
on host fibers (tests/emul/canvas_emul.cpp), the same reference, the same assertions, the gate names included.  Started
by the launcher of tests/test_emul_gpu_suite.py."""
import pytest

from tests import test_emul_gpu_suite as suite

pytestmark = pytest.mark.skipif(not suite.ENABLED,
                                reason="a real GPU is present, or the reference / mock runtime / emulation cannot be built")

NAME = "test_canvas_file_on_the_cpu"
# test -> (files, -k deselections, at least this many cases must pass): 6 model, 1 anchors, 20 sweep, 8 offsets, 2 tiny,
# 2 region views, 12 + 5 embed against the reference, 9 gravity, 15 + 12 + 1 flatten, 3 headers, 8 addalpha, 2 + 1 insert, 6 join,
# 3 + 5 + 7 second turns of the capped grids
suite.JOBS[NAME] = (["tests/test_canvas_gpu.py"], [], 128)


def test_canvas_file_on_the_cpu():
    """tests/test_canvas_gpu.py, all of it."""
    suite._run(NAME)
