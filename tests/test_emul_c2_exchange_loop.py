"""CPU: the exchange kernel's row loop (libvips_amd/csrc/reduce_fused_exch.hip: steady batches without a branch
around a load, the guarded form for a tile's head and rest) run thread by thread on host fibers (tests/emul) under
the mock HIP runtime, at four of the shapes of tests/test_c2_exchange_loop_gpu.py: the seam between the two forms
and the replicated edge column, twice in a row, bit for bit against the plain-C port."""
import os
import subprocess
import sys

import pytest

from tests import helpers
from tests.test_emul_resize_sharpen import EMUL_SO, _build_emul
from tests.test_host_glue_mock import MOCK_SO, _build_mock, _gpu_present

pytestmark = pytest.mark.skipif(_gpu_present() or not helpers.have_ref() or not _build_mock() or not _build_emul(),
                                reason="a real GPU is present, or the reference / mock runtime / emulation cannot be built")

CHILD = r'''
import sys
sys.path.insert(0, %(root)r)
import numpy as np
import libvips_amd
from libvips_amd import Image
from tests import helpers

libvips_amd.init(0)
lib = libvips_amd.lib
for (w, h) in %(cases)r:
    src = helpers.lcg_image(w, h, 4, np.uint8, 60 + w + h)
    im = Image.new_from_array(src)
    lib.vips_hip_gate_reset()
    lib.vips_hip_gate_enable(1)
    got = im.reduce(8, 8, kernel="lanczos3").numpy()
    again = im.reduce(8, 8, kernel="lanczos3").numpy()
    report = libvips_amd.gate_report()
    lib.vips_hip_gate_enable(0)
    assert sorted(report) == ["reduce_fused_u8_mfma_x"], (w, h, report)
    want = helpers.Port.reduce(src, 8, 8, "lanczos3")
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (w, h, len(bad), bad[:5])
    assert np.array_equal(again, got), (w, h)
print("CHILD-OK")
'''

# (width, height = 8 * (32 m + oh)): tiles of 32 output rows (37 groups: four steady batches and a rest), the last
# row of tiles oh rows (oh + 5 groups):
#   512 x 312    both edges in one tile; oh = 7: 12 groups, exactly the first steady batch
#   1024 x 320   a left and a right edge tile; oh = 8: one group past it
#   1536 x 344   an interior tile; oh = 11: two batches, a short rest
#   512 x 560    m = 2 (the ragged row walked top-down); oh = 6: 11 groups, one short of a steady batch
CASES = [(512, 312), (1024, 320), (1536, 344), (512, 560)]


def test_exchange_row_loop_seams(tmp_path):
    script = os.path.join(str(tmp_path), "child.py")
    with open(script, "w") as f:
        f.write(CHILD % {"root": helpers.ROOT, "cases": CASES})
    env = dict(os.environ, LD_PRELOAD=MOCK_SO, VIPS_HIP_LIBRARY=EMUL_SO, VIPS_HIP_FUSED_EXCH="1")
    proc = subprocess.run([sys.executable, script], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                          env=env, timeout=1800)
    assert proc.returncode == 0 and "CHILD-OK" in proc.stdout, proc.stdout[-3000:]
