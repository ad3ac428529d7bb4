// kern_wide_trace.hip — the traced q-split workgroup kernels of one model (mcsas_hip_plan_set_trace on a plan with more than 1024
// q-points), cold and started, for the same q slots per lane as kern_wide.hip and kern_wide_start.hip (kern_lookup.h).
#include "chain_wide.h"
#include "kern_lookup.h"
using namespace mcsas;

MCSAS_WIDE_LOOKUP(mcsas_wide_trace_kernel_m, chain_wide_trace_kernel, false)
MCSAS_WIDE_LOOKUP(mcsas_wide_trace_kernel_given_m, chain_wide_trace_kernel, true)
