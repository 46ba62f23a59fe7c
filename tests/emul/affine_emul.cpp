// TEST INFRASTRUCTURE: libvips_amd/csrc/affine.hip ITSELF (the kernel of vips_affine: the replayed coordinate walk, the clip, the
// fetch through the six extend modes, the three interpolators of interp_device.h) compiled for host fibers
// (kernel_prelude.h); takes the place of affine.hip in libvipship_emul.so.
#include "kernel_prelude.h"

#include "../../libvips_amd/csrc/affine.hip"
