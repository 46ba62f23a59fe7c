// TEST INFRASTRUCTURE: libvips_amd/csrc/recomb.hip ITSELF (vips_recomb: the streaming kernel of the fixed band counts and
// the one-pel-a-lane kernel) compiled for host fibers (kernel_prelude.h); takes the place of recomb.hip in
// libvipship_emul.so.
#include "kernel_prelude.h"

#include "../../libvips_amd/csrc/recomb.hip"
