"""CPU: tests/test_trim_gpu.py itself, run against libvipship_emul.so under the mock HIP runtime: trim.hip's kernels on
host fibers (tests/emul/trim_emul.cpp), the same reference, the same assertions, the gate names included.  Started by
the launcher of tests/test_emul_gpu_suite.py."""
import pytest

from tests import test_emul_gpu_suite as suite

pytestmark = pytest.mark.skipif(not suite.ENABLED,
                                reason="a real GPU is present, or the reference / mock runtime / emulation cannot be built")

NAME = "test_trim_file_on_the_cpu"
# test -> (files, -k deselections, at least this many cases must pass): the 161 cases of the file, as observed (40 + 40 sweeps,
# 8 over the grid, 1 + 1 + 2 + 2 + 1 project, 1 + 2 profile, 16 + 1 getpoint, 8 + 3 + 2 + 25 + 1 + 2 + 2 + 3 find_trim)
suite.JOBS[NAME] = (["tests/test_trim_gpu.py"], [], 161)


def test_trim_file_on_the_cpu():
    """tests/test_trim_gpu.py, all of it."""
    suite._run(NAME)
