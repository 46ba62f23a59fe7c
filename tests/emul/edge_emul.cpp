// TEST INFRASTRUCTURE: libvips_amd/csrc/edge.hip ITSELF (the fused uchar kernel of sobel / scharr / prewitt on the halo tile of
// nbhd_tile.h, both masks in the kernel arguments, and the general tier's combine) compiled for host fibers
// (kernel_prelude.h); takes the place of edge.hip in libvipship_emul.so.
#include "kernel_prelude.h"

#include "../../libvips_amd/csrc/edge.hip"
