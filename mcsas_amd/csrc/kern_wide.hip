// kern_wide.hip — the q-split workgroup kernels (more than 1024 q-points) of one model (kern_lookup.h).
#include "chain_wide.h"
#include "kern_lookup.h"
using namespace mcsas;

MCSAS_WIDE_LOOKUP(mcsas_wide_kernel_m, chain_wide_kernel, false)
