// TEST INFRASTRUCTURE: libvips_amd/csrc/mapim.hip ITSELF (the gather of vips_mapim through the index image and the six
// extend modes, its bounds pass and vips_xyz) compiled for host fibers (kernel_prelude.h); takes the place of mapim.hip
// in libvipship_emul.so.  The integer atomic min / max of the bounds pass, with their host meanings.
#include "kernel_prelude.h"

static inline int atomicMin(int *p, int v) { return __atomic_fetch_min(p, v, __ATOMIC_SEQ_CST); }
static inline int atomicMax(int *p, int v) { return __atomic_fetch_max(p, v, __ATOMIC_SEQ_CST); }

#include "../../libvips_amd/csrc/mapim.hip"
