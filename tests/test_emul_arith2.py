"""CPU: tests/test_arith2_gpu.py, tests/test_recomb_gpu.py and tests/test_nary_gpu.py themselves, run against
libvipship_emul.so under the mock HIP runtime: the new policies of arith.hip and the kernels of recomb.hip and nary.hip on
host fibers (tests/emul/arith_emul.cpp, recomb_emul.cpp, nary_emul.cpp), the same reference, the same assertions, the gate
names included.  Started by the launcher of tests/test_emul_gpu_suite.py."""
import pytest

from tests import test_emul_gpu_suite as suite

pytestmark = pytest.mark.skipif(not suite.ENABLED,
                                reason="a real GPU is present, or the reference / mock runtime / emulation cannot be built")

# test -> (files, -k deselections, at least this many cases must pass)
# 12 round + 1, 16 sign, 16 clamp, 32 + 3 + 1 pairs, 16 + 16 + 1 remainder, 1 refusals, 3 region forms
ARITH2 = "test_arith2_file_on_the_cpu"
suite.JOBS[ARITH2] = (["tests/test_arith2_gpu.py"], [], 118)
# 18 stream shapes, 3 forced, 4 general shapes, 8 formats, 2 order, 1 extremes, 4 matrix images, 1 refusals, 3 region forms,
# 2 + 2 + 3 second turns of the capped grids
RECOMB = "test_recomb_file_on_the_cpu"
suite.JOBS[RECOMB] = (["tests/test_recomb_gpu.py"], [], 51)
# 8 + 16 + 2 + 1 sum, 10 + 12 + 16 + 2 + 1 bandrank, 1 seventeen, 2 + 4 + 2 + 2 second turns of the capped grids
NARY = "test_nary_file_on_the_cpu"
suite.JOBS[NARY] = (["tests/test_nary_gpu.py"], [], 79)


def test_arith2_file_on_the_cpu():
    """tests/test_arith2_gpu.py, all of it."""
    suite._run(ARITH2)


def test_recomb_file_on_the_cpu():
    """tests/test_recomb_gpu.py, all of it."""
    suite._run(RECOMB)


def test_nary_file_on_the_cpu():
    """tests/test_nary_gpu.py, all of it."""
    suite._run(NARY)
