// TEST INFRASTRUCTURE: libvips_amd/csrc/reduce_fused_u8x3.hip ITSELF -- the fused vips_reduce and vips_reduceh by 8 on three interleaved uchar bands, on the matrix
// instruction -- compiled for
// host fibers (kernel_prelude.h); takes the place of reduce_fused_u8x3.hip in libvipship_emul.so.
#include "kernel_prelude.h"

#include "../../libvips_amd/csrc/reduce_fused_u8x3.hip"
