// TEST INFRASTRUCTURE: libvips_amd/csrc/reduce_fused_exch.hip ITSELF -- the fused vips_reduce of BASELINE config 2 on the matrix instruction, tiles without halos that
// exchange partial sums -- compiled for
// host fibers (kernel_prelude.h); takes the place of reduce_fused_exch.hip in libvipship_emul.so.
#include "kernel_prelude.h"

#include "../../libvips_amd/csrc/reduce_fused_exch.hip"
