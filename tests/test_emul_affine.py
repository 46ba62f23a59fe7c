"""CPU: tests/test_affine_gpu.py itself, run against libvipship_emul.so under the mock HIP runtime: the kernel of
affine.hip on host fibers (tests/emul/affine_emul.cpp), the same reference, the same assertions, the gate names
included.  Started by the launcher of tests/test_emul_gpu_suite.py."""
import pytest

from tests import test_emul_gpu_suite as suite

pytestmark = pytest.mark.skipif(not suite.ENABLED,
                                reason="a real GPU is present, or the reference / mock runtime / emulation cannot be built")

NAME = "test_affine_file_on_the_cpu"
# test -> (files, -k deselections, at least this many cases must pass): 14 matrices, 6 formats, 1 of index images,
# 3 + 3 of oarea and the displacements, 1 of backgrounds, 6 extend modes, 6 of alpha, 4 of the grid, 9 of regions,
# 1 of errors (the module's cases need the module's own library)
suite.JOBS[NAME] = (["tests/test_affine_gpu.py"], [], 54)


def test_affine_file_on_the_cpu():
    """tests/test_affine_gpu.py, all of it but the libvips module's cases."""
    suite._run(NAME)
