"""CPU: tests/test_regions_gpu.py itself, run against libvipship_emul.so under the mock HIP runtime: regions.hip's
kernels on host fibers (tests/emul/regions_emul.cpp), the same reference, the same assertions, the gate names included.
Started by the launcher of tests/test_emul_gpu_suite.py."""
import pytest

from tests import test_emul_gpu_suite as suite

pytestmark = pytest.mark.skipif(not suite.ENABLED,
                                reason="a real GPU is present, or the reference / mock runtime / emulation cannot be built")

NAME = "test_regions_file_on_the_cpu"
# test -> (files, -k deselections, at least this many cases must pass): the 52 cases of the file (4 + 1 + 2 + 1 + 4 + 15 + 5
# + 1 + 1 + 1 labelregions, 1 + 5 + 8 + 1 + 1 countlines, 1 of refusals)
suite.JOBS[NAME] = (["tests/test_regions_gpu.py"], [], 52)


def test_regions_file_on_the_cpu():
    """tests/test_regions_gpu.py, all of it."""
    suite._run(NAME)
