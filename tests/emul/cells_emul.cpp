// TEST INFRASTRUCTURE: libvips_amd/csrc/cells.hip ITSELF (vips_arrayjoin / vips_replicate / vips_wrap / vips_grid: the streaming
// and the one-pel-a-lane cells kernels) compiled for host fibers (kernel_prelude.h); takes the place of cells.hip in
// libvipship_emul.so.
#include "kernel_prelude.h"

#include "../../libvips_amd/csrc/cells.hip"
