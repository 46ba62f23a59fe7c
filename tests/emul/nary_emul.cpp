// TEST INFRASTRUCTURE: libvips_amd/csrc/nary.hip ITSELF (vips_sum and vips_bandrank over an array of images: the streaming
// and the one-element-a-lane kernels) compiled for host fibers (kernel_prelude.h); takes the place of nary.hip in
// libvipship_emul.so.
#include "kernel_prelude.h"

#include "../../libvips_amd/csrc/nary.hip"
