// TEST INFRASTRUCTURE: libvips_amd/csrc/attention.hip ITSELF (the point-wise chain and the arg-max of
// vips_smartcrop's attention search) compiled for host fibers (kernel_prelude.h); takes the place of attention.hip
// in libvipship_emul.so.
#include "kernel_prelude.h"

#include "../../libvips_amd/csrc/attention.hip"
