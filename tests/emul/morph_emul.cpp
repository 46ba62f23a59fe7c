// TEST INFRASTRUCTURE: libvips_amd/csrc/morph.hip ITSELF (erode / dilate on packed dwords: funnel-shifted reads of the halo tile of
// nbhd_tile.h, the mask as bit rows in the kernel arguments) compiled for host fibers (kernel_prelude.h); takes
// the place of morph.hip in libvipship_emul.so.
#include "kernel_prelude.h"

#include "../../libvips_amd/csrc/morph.hip"
