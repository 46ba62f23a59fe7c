"""CPU: tests/test_mapim_gpu.py itself, run against libvipship_emul.so under the mock HIP runtime: mapim.hip's gather, its
bounds pass and xyz on host fibers (tests/emul/mapim_emul.cpp), the same reference, the same assertions, the gate names
included.  Started by the launcher of tests/test_emul_gpu_suite.py."""
import pytest

from tests import test_emul_gpu_suite as suite

pytestmark = pytest.mark.skipif(not suite.ENABLED,
                                reason="a real GPU is present, or the reference / mock runtime / emulation cannot be built")

NAME = "test_mapim_file_on_the_cpu"
# test -> (files, -k deselections, at least this many cases must pass): 180 + 1 of the coordinate stage, 35 image formats,
# 8 alpha, 4 index sizes, 3 scattered, 3 + 1 + 4 region cases, 2 errors, 1 refusals, 3 xyz, 1 pipeline, 2 + 1 second turns
suite.JOBS[NAME] = (["tests/test_mapim_gpu.py"], [], 249)


def test_mapim_file_on_the_cpu():
    """tests/test_mapim_gpu.py, all of it."""
    suite._run(NAME)
