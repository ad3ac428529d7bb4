// kern_wave_sets_shared.hip — the wave-per-chain kernels of one model that fit several data sets with one population and ONE scale for
// all of them (chain_sets.h: chain_sets_kernel<M, QPL, true>; mcsas_hip_analyse_sets_mode with MCSAS_SETS_SCALE_SHARED): the shapes of
// kern_wave_sets.hip, in an object of their own beside it.
#include "chain_sets.h"
#include "kern_lookup.h"
using namespace mcsas;

void *CAT(mcsas_wave_sets_shared_kernel_m, MCSAS_M)(int qpl, bool) {
    switch (qpl) {
        case 1: return (void *)chain_sets_kernel<MCSAS_M, 1, true>;
        case 2: return (void *)chain_sets_kernel<MCSAS_M, 2, true>;
        case 4: return (void *)chain_sets_kernel<MCSAS_M, 4, true>;
        case 8: return (void *)chain_sets_kernel<MCSAS_M, 8, true>;
        case 16: return (void *)chain_sets_kernel<MCSAS_M, 16, true>;
        default: return nullptr;
    }
}
