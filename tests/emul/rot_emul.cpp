// TEST INFRASTRUCTURE: libvips_amd/csrc/rot.hip ITSELF (vips_rot / vips_flip / vips_autorot: the transposing tile
// kernel, the streaming flips, the one-pel-a-lane kernel) compiled for host fibers (kernel_prelude.h); takes the place
// of rot.hip in libvipship_emul.so.
#include "kernel_prelude.h"

#include "../../libvips_amd/csrc/rot.hip"
