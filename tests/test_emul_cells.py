"""CPU: tests/test_cells_gpu.py itself, run against libvipship_emul.so under the mock HIP runtime: cells.hip's kernels
on host fibers (tests/emul/cells_emul.cpp), the same reference, the same assertions, the gate names included.  Started
by the launcher of tests/test_emul_gpu_suite.py."""
import pytest

from tests import test_emul_gpu_suite as suite

pytestmark = pytest.mark.skipif(not suite.ENABLED,
                                reason="a real GPU is present, or the reference / mock runtime / emulation cannot be built")

NAME = "test_cells_file_on_the_cpu"
# test -> (files, -k deselections, at least this many cases must pass): 4 + 1 model, 1 anchors, 20 + 2 + 2 sweep, 20 + 2
# replicate, 2 clamp, 2 cropping, 2 + 1 against the reference, 1 zoom / subsample, 2 + 2 regions, 1 refusals (the
# module's three need the module's own library, the two-device case two devices), 2 + 5 + 4 second turns of the capped grids
suite.JOBS[NAME] = (["tests/test_cells_gpu.py"], [], 76)


def test_cells_file_on_the_cpu():
    """tests/test_cells_gpu.py, all of it but the libvips module's cases."""
    suite._run(NAME)
