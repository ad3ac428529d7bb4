// kern_wave_start.hip — instantiates the start forms of the wave-per-chain kernels (chain_wave_start_kernel and
// chain_wave_batch_start_kernel: the first attempt takes a given set, mcsas_hip_plan_set_start) for ONE model (-DMCSAS_M=<id>), for
// the same q-slot / row-cache pairs as kern_wave.hip and kern_wave_batch.hip.  Exports the lookups the host code links against.
#include "chain_wave.h"
#ifndef MCSAS_M
#error "compile with -DMCSAS_M=<model id>"
#endif
#define CAT_(a, b) a##b
#define CAT(a, b) CAT_(a, b)
using namespace mcsas;

template <int QPL> static void *pick(bool cache) {
    return cache ? (void *)chain_wave_start_kernel<MCSAS_M, QPL, true> : (void *)chain_wave_start_kernel<MCSAS_M, QPL, false>;
}
template <int QPL> static void *pick_batch(bool cache) {
    return cache ? (void *)chain_wave_batch_start_kernel<MCSAS_M, QPL, true> : (void *)chain_wave_batch_start_kernel<MCSAS_M, QPL, false>;
}
void *CAT(mcsas_wave_start_kernel_m, MCSAS_M)(int qpl, bool cache) {
    switch (qpl) {
        case 1: return pick<1>(cache);
        case 2: return pick<2>(cache);
        case 4: return pick<4>(cache);
        case 8: return pick<8>(cache);
        case 16: return pick<16>(cache);
        case 32: return cache ? (void *)chain_wave_start_kernel<MCSAS_M, 32, true> : nullptr;
        case 64: return cache ? (void *)chain_wave_start_kernel<MCSAS_M, 64, true> : nullptr;
        default: return nullptr;
    }
}
void *CAT(mcsas_wave_batch_start_kernel_m, MCSAS_M)(int qpl, bool cache) {
    switch (qpl) {
        case 1: return pick_batch<1>(cache);
        case 2: return pick_batch<2>(cache);
        case 4: return pick_batch<4>(cache);
        case 8: return pick_batch<8>(cache);
        case 16: return pick_batch<16>(cache);
        case 32: return cache ? (void *)chain_wave_batch_start_kernel<MCSAS_M, 32, true> : nullptr;
        case 64: return cache ? (void *)chain_wave_batch_start_kernel<MCSAS_M, 64, true> : nullptr;
        default: return nullptr;
    }
}
