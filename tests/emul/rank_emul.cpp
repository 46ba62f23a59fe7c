// TEST INFRASTRUCTURE: libvips_amd/csrc/rank.hip ITSELF (the three kernels of vips_rank: the 3 x 3 median network, the separable
// minimum / maximum, the bisection select, on the halo tile of nbhd_tile.h) compiled for host fibers (kernel_prelude.h); takes
// the place of rank.hip in libvipship_emul.so.
#include "kernel_prelude.h"

#include "../../libvips_amd/csrc/rank.hip"
