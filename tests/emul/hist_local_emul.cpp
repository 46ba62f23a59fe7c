// TEST INFRASTRUCTURE: libvips_amd/csrc/hist_local.hip ITSELF (vips_hist_local: the counting kernel and the sliding
// histograms, a lane's own 16-bit bins in LDS under LDS atomic adds, on the mirrored halo tile of nbhd_tile.h;
// vips_stdif: column sums in LDS, the doubles of stdif.c) compiled for host fibers (kernel_prelude.h); takes the place
// of hist_local.hip in libvipship_emul.so.
#include "kernel_prelude.h"

#include "../../libvips_amd/csrc/hist_local.hip"
