// TEST INFRASTRUCTURE: libvips_amd/csrc/logic.hip ITSELF (vips_relational / vips_boolean and their _const forms,
// vips_ifthenelse, vips_bandjoin / vips_extract_band / vips_bandmean / vips_bandbool: the streaming and the
// one-element-a-lane kernels) compiled for host fibers (kernel_prelude.h); takes the place of logic.hip in
// libvipship_emul.so.
#include "kernel_prelude.h"

#include "../../libvips_amd/csrc/logic.hip"
