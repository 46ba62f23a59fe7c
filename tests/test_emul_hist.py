"""CPU: tests/test_hist_gpu.py itself, run against libvipship_emul.so under the mock HIP runtime: maplut_u8 of hist.hip
and the kernels of hist_local.hip on host fibers (tests/emul/hist_emul.cpp, hist_local_emul.cpp), the same reference,
the same assertions, the gate names included.  Started by the launcher of tests/test_emul_gpu_suite.py."""
import pytest

from tests import test_emul_gpu_suite as suite

pytestmark = pytest.mark.skipif(not suite.ENABLED,
                                reason="a real GPU is present, or the reference / mock runtime / emulation cannot be built")

NAME = "test_hist_file_on_the_cpu"
# test -> (files, -k deselections, at least this many cases must pass): 3 + 1 of hist_cum / hist_norm, 3 + 1 of
# hist_equal, 8 + 3 + 1 + 1 + 1 of maplut, 10 + 1 + 3 + 3 + 1 of hist_local, 7 + 3 + 1 + 1 + 1 of stdif, 4 + 3 region
# cases (the module's three need the module's own library), 2 second turns of maplut, 1 tall-image guard of stdif
suite.JOBS[NAME] = (["tests/test_hist_gpu.py"], [], 63)


def test_hist_file_on_the_cpu():
    """tests/test_hist_gpu.py, all of it but the libvips module's cases."""
    suite._run(NAME)
