// kern_lookup.h — what the kern_*.hip units share: each instantiates one family's kernels for ONE model (-DMCSAS_M=<id>), so that
// the models build in parallel, and exports a lookup `void *(int qpl, bool flag)` the host code links against (mcsas_hip.hip:
// BUILTIN).  flag: the family's own (row cache / row queue); the families without one ignore it.  Here are the qpl -> instance
// tables of the two families that come cold and started (GIVEN: chain_body.inc), written once; a unit names its kernel template
// and its GIVEN.  Not among the texts of the plug-in compiler: a plug-in names its one instance itself (host_plugin.hip).
#pragma once
#ifndef MCSAS_M
#error "compile with -DMCSAS_M=<model id>"
#endif
#define CAT_(a, b) a##b
#define CAT(a, b) CAT_(a, b)

// one wavefront per chain, KERNEL<M, QPL, CACHE, GIVEN> (chain_wave.h); PICK names the unit's helper template
#define MCSAS_WAVE_LOOKUP(LOOKUP, PICK, KERNEL, GIVEN)                                                                              \
    template <int QPL> static void *PICK(bool cache) {                                                                             \
        return cache ? (void *)KERNEL<MCSAS_M, QPL, true, GIVEN> : (void *)KERNEL<MCSAS_M, QPL, false, GIVEN>;                     \
    }                                                                                                                              \
    void *CAT(LOOKUP, MCSAS_M)(int qpl, bool cache) {                                                                              \
        switch (qpl) {                                                                                                             \
            case 1: return PICK<1>(cache);                                                                                         \
            case 2: return PICK<2>(cache);                                                                                         \
            case 4: return PICK<4>(cache);                                                                                         \
            case 8: return PICK<8>(cache);                                                                                         \
            case 16: return PICK<16>(cache);                                                                                       \
            /* nq up to 2048 / 4096 (un-binned data files, nBin = 0): cached rows only — the host forces the cache on */           \
            case 32: return cache ? (void *)KERNEL<MCSAS_M, 32, true, GIVEN> : nullptr;                                            \
            case 64: return cache ? (void *)KERNEL<MCSAS_M, 64, true, GIVEN> : nullptr;                                            \
            default: return nullptr;                                                                                               \
        }                                                                                                                          \
    }

// the q-split workgroup, KERNEL<M, QPL, GIVEN> (chain_wide.h): 8 waves x 64 lanes x QPL q-points
#define MCSAS_WIDE_LOOKUP(LOOKUP, KERNEL, GIVEN)                                                                                    \
    void *CAT(LOOKUP, MCSAS_M)(int qpl, bool) {                                                                                    \
        switch (qpl) {                                                                                                             \
            case 8: return (void *)KERNEL<MCSAS_M, 8, GIVEN>;   /* up to 4096 q-points */                                          \
            case 16: return (void *)KERNEL<MCSAS_M, 16, GIVEN>; /* up to 8192 */                                                   \
            case 32: return (void *)KERNEL<MCSAS_M, 32, GIVEN>; /* up to 16384 */                                                  \
            default: return nullptr;                                                                                               \
        }                                                                                                                          \
    }
