// TEST INFRASTRUCTURE: libvips_amd/csrc/hist.hip ITSELF (the histograms of up to six rectangles in one launch: a
// wave's own counters in LDS, LDS and global atomic adds) compiled for host fibers (kernel_prelude.h); takes the
// place of hist.hip in libvipship_emul.so.
#include "kernel_prelude.h"

#include "../../libvips_amd/csrc/hist.hip"
