// TEST INFRASTRUCTURE: libvips_amd/csrc/correlation.hip ITSELF (vips_fastcor and vips_spcor: the staged halo tile, the
// serial sums in the reference's order) compiled for host fibers (kernel_prelude.h); takes the place of correlation.hip
// in libvipship_emul.so.  The kernels use nothing the prelude lacks: sqrt is the host's, correctly rounded as the
// device's.
#include "kernel_prelude.h"

#include "../../libvips_amd/csrc/correlation.hip"
