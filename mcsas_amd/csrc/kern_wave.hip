// kern_wave.hip — the wave-per-chain kernels of one model (kern_lookup.h).
#include "chain_wave.h"
#include "kern_lookup.h"
using namespace mcsas;

MCSAS_WAVE_LOOKUP(mcsas_wave_kernel_m, pick, chain_wave_kernel, false)
