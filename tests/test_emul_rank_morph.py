"""CPU: tests/test_rank_morph_gpu.py itself, run against libvipship_emul.so under the mock HIP runtime: the kernels of
rank.hip and morph.hip on host fibers (tests/emul/rank_emul.cpp, morph_emul.cpp), the same reference, the same
assertions, the gate names included.  Started by the launcher of tests/test_emul_gpu_suite.py."""
import pytest

from tests import test_emul_gpu_suite as suite

pytestmark = pytest.mark.skipif(not suite.ENABLED,
                                reason="a real GPU is present, or the reference / mock runtime / emulation cannot be built")

NAME = "test_rank_morph_file_on_the_cpu"
# test -> (files, -k deselections, at least this many cases must pass): 11 windows, 3 + 6 + 1 + 3 + 3 rank cases,
# 9 + 1 + 3 + 2 morph cases, 4 + 3 + 1 region cases, 1 of errors (the module's three need the module's own library)
suite.JOBS[NAME] = (["tests/test_rank_morph_gpu.py"], [], 51)


def test_rank_morph_file_on_the_cpu():
    """tests/test_rank_morph_gpu.py, all of it but the libvips module's cases."""
    suite._run(NAME)
