// kern_wave_batch.hip — the batch form of the wave-per-chain kernel (several analyses in one launch) of one model, for the same
// q-slot / row-cache pairs as kern_wave.hip (kern_lookup.h).
#include "chain_wave.h"
#include "kern_lookup.h"
using namespace mcsas;

MCSAS_WAVE_LOOKUP(mcsas_wave_batch_kernel_m, pick, chain_wave_batch_kernel, false)
