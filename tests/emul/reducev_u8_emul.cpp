// TEST INFRASTRUCTURE: libvips_amd/csrc/reducev_u8.hip ITSELF -- the one-axis vertical uchar kernels (reducev on the matrix instruction and on the vector
// ALU, shrinkv) -- compiled for
// host fibers (kernel_prelude.h); takes the place of reducev_u8.hip in libvipship_emul.so.
#include "kernel_prelude.h"

#include "../../libvips_amd/csrc/reducev_u8.hip"
