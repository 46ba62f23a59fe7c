// TEST INFRASTRUCTURE: libvips_amd/csrc/reduce_fused_u8.hip ITSELF -- the fused vips_reduce on RGBA uchar, on the vector ALU and -- tiles with halos -- on the matrix
// instruction (v_mfma_f32_4x4x4_16b_f16 and the quad DPP moves as wave meetings of the fibers), and its entry point -- compiled for
// host fibers (kernel_prelude.h); takes the place of reduce_fused_u8.hip in libvipship_emul.so.
#include "kernel_prelude.h"

#include "../../libvips_amd/csrc/reduce_fused_u8.hip"
