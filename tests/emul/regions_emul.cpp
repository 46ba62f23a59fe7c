// TEST INFRASTRUCTURE: libvips_amd/csrc/regions.hip ITSELF (vips_labelregions' six passes and vips_countlines) compiled
// for host fibers (kernel_prelude.h); takes the place of regions.hip in libvipship_emul.so.  The integer atomics the
// file uses -- the LDS min, the agent-scope load and min on the parent plane, the 64-bit add -- with their host meanings.
#include "kernel_prelude.h"

static inline int atomicMin(int *p, int v) { return __atomic_fetch_min(p, v, __ATOMIC_SEQ_CST); }
static inline unsigned long long atomicAdd(unsigned long long *p, unsigned long long v) { return __atomic_fetch_add(p, v, __ATOMIC_SEQ_CST); }
#ifndef __HIP_MEMORY_SCOPE_AGENT
#define __HIP_MEMORY_SCOPE_AGENT 4
#endif
#define __hip_atomic_load(p, order, scope) __atomic_load_n((p), (order))
#define __hip_atomic_fetch_min(p, v, order, scope) __atomic_fetch_min((p), (v), (order))

#include "../../libvips_amd/csrc/regions.hip"
