"""CPU: tests/test_arith_gpu.py itself, run against libvipship_emul.so under the mock HIP runtime: arith.hip's kernels on
host fibers (tests/emul/arith_emul.cpp), the same reference, the same assertions, the gate names included.  Started by
the launcher of tests/test_emul_gpu_suite.py."""
import pytest

from tests import test_emul_gpu_suite as suite

pytestmark = pytest.mark.skipif(not suite.ENABLED,
                                reason="a real GPU is present, or the reference / mock runtime / emulation cannot be built")

NAME = "test_arith_file_on_the_cpu"
# test -> (files, -k deselections, at least this many cases must pass): 6 + 2 + 12 linear on domains, 1 errors and
# operators, 16 + 1 invert / abs, 60 + 8 + 20 sweeps, 1 models, 4 + 1 whole images, 8 + 4 + 24 + 4 + 7 two images, 50 + 4 + 1 + 2 + 2 + 2 + 1 stats (the
# 3 module cases need the module's own library), 3 + 3 second turns of the capped grids
suite.JOBS[NAME] = (["tests/test_arith_gpu.py"], [], 247)


def test_arith_file_on_the_cpu():
    """tests/test_arith_gpu.py, all of it."""
    suite._run(NAME)
