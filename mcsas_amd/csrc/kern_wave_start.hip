// kern_wave_start.hip — the wave-per-chain kernels of one model, single and batch, whose first attempt takes a given set
// (mcsas_hip_plan_set_start; GIVEN), for the same q-slot / row-cache pairs as kern_wave.hip and kern_wave_batch.hip (kern_lookup.h).
#include "chain_wave.h"
#include "kern_lookup.h"
using namespace mcsas;

MCSAS_WAVE_LOOKUP(mcsas_wave_kernel_given_m, pick, chain_wave_kernel, true)
MCSAS_WAVE_LOOKUP(mcsas_wave_batch_kernel_given_m, pick_batch, chain_wave_batch_kernel, true)
