// kern_wide_start.hip — the q-split workgroup kernels of one model whose first attempt takes a given set (mcsas_hip_plan_set_start;
// GIVEN), for the same q slots per lane as kern_wide.hip (kern_lookup.h).
#include "chain_wide.h"
#include "kern_lookup.h"
using namespace mcsas;

MCSAS_WIDE_LOOKUP(mcsas_wide_kernel_given_m, chain_wide_kernel, true)
