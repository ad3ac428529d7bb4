// kern_wave_trace.hip — the traced wave-per-chain kernels of one model (mcsas_hip_plan_set_trace), cold and started, for the same
// q-slot / row-cache pairs as kern_wave.hip and kern_wave_start.hip (kern_lookup.h).
#include "chain_wave.h"
#include "kern_lookup.h"
using namespace mcsas;

MCSAS_WAVE_LOOKUP(mcsas_wave_trace_kernel_m, pick, chain_wave_trace_kernel, false)
MCSAS_WAVE_LOOKUP(mcsas_wave_trace_kernel_given_m, pick_given, chain_wave_trace_kernel, true)
