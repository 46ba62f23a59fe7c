"""CPU: tests/test_edge_gpu.py itself, run against libvipship_emul.so under the mock HIP runtime: the kernels of
edge.hip on host fibers (tests/emul/edge_emul.cpp), the same reference, the same assertions, the gate names
included.  Started by the launcher of tests/test_emul_gpu_suite.py."""
import pytest

from tests import test_emul_gpu_suite as suite

pytestmark = pytest.mark.skipif(not suite.ENABLED,
                                reason="a real GPU is present, or the reference / mock runtime / emulation cannot be built")

NAME = "test_edge_file_on_the_cpu"
# test -> (files, -k deselections, at least this many cases must pass): 19 of sobel / scharr / prewitt, 3 + 3 + 1 + 3 +
# 5 + 1 + 3 of compass, 3 + 3 + 2 + 4 + 1 + 1 of canny, 4 of the region forms' and refusals' rest (the module's three
# need the module's own library), 3 + 3 second turns of the combining kernels
suite.JOBS[NAME] = (["tests/test_edge_gpu.py"], [], 66)


def test_edge_file_on_the_cpu():
    """tests/test_edge_gpu.py, all of it but the libvips module's cases."""
    suite._run(NAME)
