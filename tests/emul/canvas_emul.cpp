// TEST INFRASTRUCTURE: libvips_amd/csrc/canvas.hip ITSELF (vips_embed / vips_gravity / vips_insert / vips_join: the streaming
// and the one-pel-a-lane canvas kernels; vips_flatten and vips_addalpha) compiled for host fibers (kernel_prelude.h); takes
// the place of canvas.hip in libvipship_emul.so.
#include "kernel_prelude.h"

#include "../../libvips_amd/csrc/canvas.hip"
