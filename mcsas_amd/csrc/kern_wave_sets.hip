// kern_wave_sets.hip — the wave-per-chain kernels of one model that fit several data sets with one population (chain_sets.h;
// mcsas_hip_analyse_sets): cached rows only, 1 to 16 q slots per lane (the padded sets together take up to 1024 entries).
#include "chain_sets.h"
#include "kern_lookup.h"
using namespace mcsas;

void *CAT(mcsas_wave_sets_kernel_m, MCSAS_M)(int qpl, bool) {
    switch (qpl) {
        case 1: return (void *)chain_sets_kernel<MCSAS_M, 1>;
        case 2: return (void *)chain_sets_kernel<MCSAS_M, 2>;
        case 4: return (void *)chain_sets_kernel<MCSAS_M, 4>;
        case 8: return (void *)chain_sets_kernel<MCSAS_M, 8>;
        case 16: return (void *)chain_sets_kernel<MCSAS_M, 16>;
        default: return nullptr;
    }
}
