// TEST INFRASTRUCTURE: libvips_amd/csrc/arith.hip ITSELF (vips_linear / vips_invert / vips_abs, vips_add / vips_subtract /
// vips_multiply / vips_divide: the streaming and the one-element-a-lane kernels; the scan of vips_stats) compiled for host
// fibers (kernel_prelude.h); takes the place of arith.hip in libvipship_emul.so.
#include "kernel_prelude.h"

#include "../../libvips_amd/csrc/arith.hip"
