"""CPU: tests/test_correlation_gpu.py itself, run against libvipship_emul.so under the mock HIP runtime: correlation.hip's
fastcor and spcor kernels and the statistics scan of uint and int images on host fibers (tests/emul/correlation_emul.cpp),
the same reference, the same assertions, the gate names included.  Started by the launcher of
tests/test_emul_gpu_suite.py."""
import pytest

from tests import test_emul_gpu_suite as suite

pytestmark = pytest.mark.skipif(not suite.ENABLED,
                                reason="a real GPU is present, or the reference / mock runtime / emulation cannot be built")

NAME = "test_correlation_file_on_the_cpu"
# test -> (files, -k deselections, at least this many cases must pass): 64 formats, 6 seams, 16 small, 4 + 2 largest ref,
# 8 + 2 band matching, 6 format matching, 3 + 2 + 8 of spcor, 1 + 2 of fastcor, 2 refusals, 4 + 4 + 1 + 1 extremes,
# 3 end to end
suite.JOBS[NAME] = (["tests/test_correlation_gpu.py"], [], 139)


def test_correlation_file_on_the_cpu():
    """tests/test_correlation_gpu.py, all of it."""
    suite._run(NAME)
