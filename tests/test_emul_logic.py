"""CPU: tests/test_logic_gpu.py itself, run against libvipship_emul.so under the mock HIP runtime: logic.hip's kernels on
host fibers (tests/emul/logic_emul.cpp), the same reference, the same assertions, the gate names included.  Started by
the launcher of tests/test_emul_gpu_suite.py."""
import pytest

from tests import test_emul_gpu_suite as suite

pytestmark = pytest.mark.skipif(not suite.ENABLED,
                                reason="a real GPU is present, or the reference / mock runtime / emulation cannot be built")

NAME = "test_logic_file_on_the_cpu"
# test -> (files, -k deselections, at least this many cases must pass): the 643 cases of the file that need no module library, as observed (12 + 42 + 48 +
# 1 relational, 10 + 35 + 40 + 1 boolean, 6 + 1 matching, 16 + 1 + 1 ifthenelse, 1 + 8 + 8 + 1 bands, 360 + 8 + 40 + 1 sweeps, 2 errors
# and operators), 3 + 6 second turns of the capped grids
suite.JOBS[NAME] = (["tests/test_logic_gpu.py"], [], 652)


def test_logic_file_on_the_cpu():
    """tests/test_logic_gpu.py, all of it."""
    suite._run(NAME)
