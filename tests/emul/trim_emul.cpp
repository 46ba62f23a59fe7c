// TEST INFRASTRUCTURE: libvips_amd/csrc/trim.hip ITSELF (vips_project, vips_profile and the fused scan of vips_find_trim:
// the streaming and the one-element-a-lane kernels) compiled for host fibers (kernel_prelude.h); takes the place of
// trim.hip in libvipship_emul.so.  The integer atomic min / max and the fence the file uses, with their host meanings.
#include "kernel_prelude.h"

static inline int atomicMin(int *p, int v) { return __atomic_fetch_min(p, v, __ATOMIC_SEQ_CST); }
static inline unsigned int atomicMax(unsigned int *p, unsigned int v) { return __atomic_fetch_max(p, v, __ATOMIC_SEQ_CST); }
#define __threadfence() __atomic_thread_fence(__ATOMIC_SEQ_CST)

#include "../../libvips_amd/csrc/trim.hip"
