// chain_wave.h — one wavefront = one Monte-Carlo chain (McSAS.mcFit, mcsas.py:287-439), all
// attempts of one repetition (the retry loop of McSAS.analyse, mcsas.py:220-246).
//
// Layout: q index i lives in lane (i & 63), register slot (i >> 6); QPL = slots per lane.
//   registers : ft[QPL] (running model intensity), per-step new/old/test rows
//   LDS       : q, w = 1/sigma^2, wI = I/sigma^2 (read-only, shared by the block), orientation table
//   HBM       : rset[N][P], cached per-contribution intensity rows [N][qpad] (CACHE), outputs
// No barriers in the step loop: the three weighted sums are reduced with DPP inside the wave,
// the accept/reject decision is wave-uniform.  The chain itself is chain_body.inc, shared with chain_wide.h; the kernels below
// differ in how they come by their analysis, and chain_wave_kernel.inc is what they do with it.
#pragma once
#include "chain_common.h"

namespace mcsas {

// waves per SIMD the chain kernels are built for (the batch kernel below keeps its single twin's)
#define MCSAS_WAVE_MIN_WAVES(QPL, CACHE) (((QPL) < 8 || ((QPL) == 8 && (CACHE))) ? 2 : 1)

// the trace hooks of chain_wave_kernel.inc: nothing in the kernels of this file, except in chain_wave_trace_kernel
#define MCSAS_WAVE_TRACE_START(c)
#define MCSAS_WAVE_TRACE_MOVE(i, s, c, k)

// GIVEN: the chain is started from a given set (mcsas_hip_plan_set_start): the host has copied the repetition's start into rset
// ahead of the launch, and the first attempt takes it where the cold kernel generates one (chain_body.inc: GIVEN).
template <int M, int QPL, bool CACHE, bool GIVEN>
__global__ __launch_bounds__(64, MCSAS_WAVE_MIN_WAVES(QPL, CACHE)) void chain_wave_kernel(const ChainArgs a) {
    extern __shared__ double lds[];
    const int lane = threadIdx.x;
    const int rep = blockIdx.x;
#include "chain_wave_kernel.inc"
}

// Every pointer of an argument block points into device (or mapped host) memory, i.e. the global address space.  The compiler
// assumes that of a pointer it reads from the constant address space (a kernel argument is read from there), not of one read from
// plain memory: the pointers of the block are therefore read through a constant-space view of the table, or the chain's loads and
// stores would all be flat instructions.
typedef const __attribute__((address_space(4))) ChainArgs ConstChainArgs;
__device__ __forceinline__ void chain_args_pointers(ChainArgs &a, ConstChainArgs &c) {
    a.model.smear_locs_t = c.model.smear_locs_t; a.model.smear_cw = c.model.smear_cw;
    a.q = c.q; a.w = c.w; a.wI = c.wI; a.I = c.I;
    a.replay = c.replay; a.stop_flag = c.stop_flag; a.stop_relay = c.stop_relay;
    a.rset = c.rset; a.cache = c.cache; a.fit = c.fit; a.out = c.out;
}

// A batch of analyses (data sets) in one launch (mcsas_hip_plan_launch_batch): block b runs repetition chains[b].rep of the
// analysis sets[chains[b].set] (ChainRef: chain_common.h) with the same body.  The entry and the index are wave-uniform by
// construction; saying so (readfirstlane) lets the compiler read the argument block with scalar loads at the start, as it reads a
// kernel argument.  Both tables are read-only here: every result goes through the analysis' own output pointers.
// GIVEN: every analysis of such a launch has its start in its rset (plans with and without a start share a batch call, not a launch:
// the host groups them apart).
template <int M, int QPL, bool CACHE, bool GIVEN>
__global__ __launch_bounds__(64, MCSAS_WAVE_MIN_WAVES(QPL, CACHE)) void chain_wave_batch_kernel(const ChainArgs *__restrict__ sets,
                                                                                                const ChainRef *__restrict__ chains) {
    extern __shared__ double lds[];
    const int lane = threadIdx.x;
    const ChainRef c = chains[blockIdx.x];
    const int rep = __builtin_amdgcn_readfirstlane(c.rep);
    const int set = __builtin_amdgcn_readfirstlane(c.set);
    ChainArgs a = sets[set];                                    // (read whole before the first store)
    chain_args_pointers(a, ((ConstChainArgs *)sets)[set]);
#include "chain_wave_kernel.inc"
}

#undef MCSAS_WAVE_TRACE_START
#undef MCSAS_WAVE_TRACE_MOVE

// The traced form of chain_wave_kernel (mcsas_hip_plan_set_trace): the same chain, and lane 0 also records the accepted moves of the
// last attempt in the repetition's part of `t` (TraceArgs, chain_common.h) — the reference reports them as it goes, mcsas.py:385-390.
// An attempt's start writes the chi² of its initial set; move i of the attempt overwrites record i of the attempt before, so what is
// left at the end are the records of the last attempt (its count is ChainOut::num_moves) and, behind them, stale ones the host
// drops.  One bounds test and 2 + P stores per accepted move; nothing in a rejected step.  Nothing the chain computes reads `t`.
#define MCSAS_WAVE_TRACE_START(c) if (lane == 0) t.chisq0[rep] = c;
#define MCSAS_WAVE_TRACE_MOVE(i, s, c, k)                                                                              \
    if (i < (int64_t)t.capacity) {                                                                                     \
        const size_t rec = (size_t)rep * (size_t)t.capacity + (size_t)i;                                               \
        _Pragma("unroll") for (int p = 0; p < MCSAS_MAX_ACTIVE; ++p)                                                   \
            if (p < P) {                                                                                               \
                const double tv = readlane_f64(prow[p], k);                                                            \
                if (lane == 0) t.values[rec * P + p] = tv;                                                             \
            }                                                                                                          \
        if (lane == 0) { t.step[rec] = s; t.chisq[rec] = c; }                                                          \
    }
template <int M, int QPL, bool CACHE, bool GIVEN>
__global__ __launch_bounds__(64, MCSAS_WAVE_MIN_WAVES(QPL, CACHE)) void chain_wave_trace_kernel(const ChainArgs a, const TraceArgs t) {
    extern __shared__ double lds[];
    const int lane = threadIdx.x;
    const int rep = blockIdx.x;
#include "chain_wave_kernel.inc"
}
#undef MCSAS_WAVE_TRACE_START
#undef MCSAS_WAVE_TRACE_MOVE

}  // namespace mcsas
