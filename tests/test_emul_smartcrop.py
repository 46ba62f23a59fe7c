"""CPU: tests/test_smartcrop_gpu.py itself, run against libvipship_emul.so under the mock HIP runtime: the kernels of
hist.hip and attention.hip on host fibers (tests/emul/hist_emul.cpp, attention_emul.cpp) beside every kernel the
searches and the thumbnails go through, the same reference, the same assertions, the gate names and launch counts
included.  Started by the launcher of tests/test_emul_gpu_suite.py."""
import pytest

from tests import test_emul_gpu_suite as suite

pytestmark = pytest.mark.skipif(not suite.ENABLED,
                                reason="a real GPU is present, or the reference / mock runtime / emulation cannot be built")

NAME = "test_smartcrop_file_on_the_cpu"
# test -> (files, -k deselections, at least this many cases must pass): 4 + 4 + 1 + 1 histogram cases, 13 + 1 entropy,
# 11 + 1 attention, 5 positional, 4 + 2 thumbnails, 2 refusals, 2 + 1 second turns of the histogram kernel
suite.JOBS[NAME] = (["tests/test_smartcrop_gpu.py"], [], 52)


def test_smartcrop_file_on_the_cpu():
    """tests/test_smartcrop_gpu.py, all of it."""
    suite._run(NAME)
