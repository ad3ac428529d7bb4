// chain_wide.h — one workgroup = one Monte-Carlo chain, the q-points split over its waves: the kernel for data sets with
// more than 1024 q-points (un-binned files, nBin = 0: dataobj/dataconfig.py:99; McSAS.analyse takes any data.count,
// mcsas.py:210).  Same chain as chain_wave.h (McSAS.mcFit, mcsas.py:287-439; retry loop of McSAS.analyse, :220-246), compiled from
// the same text (chain_body.inc); what differs is where a q-point lives and how the three weighted sums of a step are put
// together, and this file holds that and nothing of the step.
//
// Layout: NW = blockDim.x / 64 waves (<= 8), qpad = 64 * QPL * NW; wave v owns the q slice [64 QPL v, 64 QPL (v + 1)):
// q index i = 64 (QPL v + j) + lane, j = register slot.  ft, w, wI of the slice live in registers; q and 1/q^3 in LDS when
// they fit beside the model's tables (ChainArgs::pad1 = 1), else they are read from HBM/L2 through the same pointers.
// Per step: every wave evaluates its slice of the proposal's row, reads its slice of the `old` row from the row cache
// (always on), reduces its three partial sums with DPP and parks them in LDS; ONE workgroup barrier; every wave adds the NW
// partials in wave order — the same numbers in every wave, so the accept/reject decision is uniform over the workgroup
// without a second exchange.  The partial slots alternate by step parity: a wave can only reach its write of step s + 2
// through the barrier of step s + 1, which every wave passes after reading step s.
//
// The file is read in passes.  The first one (no MCSAS_WIDE_PASS) declares what the kernels share and then includes this file once
// per kernel, with the kernel's name, what it takes behind q3inv_glb and its two trace hooks as MCSAS_WIDE_* macros — the way
// chain_wave_kernel.inc forwards MCSAS_WAVE_TRACE_*: chain_wide_kernel (hooks empty) and chain_wide_trace_kernel.  A kernel pass is
// the text behind `#else` below: one kernel template, the only place of this family that includes chain_body.inc.
#ifndef MCSAS_WIDE_PASS
#ifndef MCSAS_CHAIN_WIDE_H
#define MCSAS_CHAIN_WIDE_H
#include "chain_common.h"

namespace mcsas {

constexpr int WIDE_MAX_WAVES = 8;        // 2 waves per SIMD: the row evaluators keep their 256 registers (16 waves: 128, and the sphere's interleaved sincos spills)
constexpr int WIDE_PART_DOUBLES = 2 * WIDE_MAX_WAVES * 4 + 8;       // partial sums [parity][wave][4], then the stop word

// block-wide sums of three per-lane values, the same in every thread; `par` alternates per call
__device__ __forceinline__ void wide_sum3(double &s1, double &s2, double &s3, double *part, int &par, int wave, int lane, int NW) {
    wave_sum3(s1, s2, s3);
    double *slot = part + (size_t)(par * WIDE_MAX_WAVES) * 4;
    if (lane == 0) { slot[wave * 4 + 0] = s1; slot[wave * 4 + 1] = s2; slot[wave * 4 + 2] = s3; }
    __syncthreads();
    double t1 = 0., t2 = 0., t3 = 0.;
    for (int v = 0; v < NW; ++v) { t1 += slot[v * 4 + 0]; t2 += slot[v * 4 + 1]; t3 += slot[v * 4 + 2]; }
    s1 = t1; s2 = t2; s3 = t3;
    par ^= 1;
}

// ... and of one
__device__ __forceinline__ double wide_sum1(double s, double *part, int &par, int wave, int lane, int NW) {
    double z1 = 0., z2 = 0.;
    wide_sum3(s, z1, z2, part, par, wave, lane, NW);
    return s;
}

// McSAS.stop: one thread looks, everybody acts on what it saw (a wave of its own could see the word change between two waves'
// reads and leave the others at the next barrier)
__device__ __forceinline__ bool wide_stop(const ChainArgs &a, int32_t *stop_word, int tid) {
    if (!a.stop_flag) return false;
    if (tid == 0) *stop_word = stop_requested(a) ? 1 : 0;
    __syncthreads();
    return *stop_word != 0;
}

}  // namespace mcsas

#define MCSAS_WIDE_PASS
// the chain and nothing else
#define MCSAS_WIDE_KERNEL chain_wide_kernel
#define MCSAS_WIDE_TRACE_PARAM
#define MCSAS_WIDE_TRACE_START(c)
#define MCSAS_WIDE_TRACE_MOVE(i, s, c, k)
#include "chain_wide.h"
#undef MCSAS_WIDE_KERNEL
#undef MCSAS_WIDE_TRACE_PARAM
#undef MCSAS_WIDE_TRACE_START
#undef MCSAS_WIDE_TRACE_MOVE

// The traced form (mcsas_hip_plan_set_trace on a q-split plan): the same chain, and thread 0 of the workgroup also records the accepted
// moves of the last attempt in the repetition's part of `t` (TraceArgs, chain_common.h), with the semantics of chain_wave_trace_kernel
// (chain_wave.h): an attempt's start writes the chi² of its initial set; move i of the attempt overwrites record i of the attempt
// before, so what is left at the end are the records of the last attempt (its count is ChainOut::num_moves) and, behind them, stale
// ones the host drops.  One writer is enough: prow, cur.chi2, num_iter and num_moves are the same numbers in every wave (the
// proposals are, and the sums are added in wave order).  One bounds test and 2 + P stores per accepted move; nothing in a rejected
// step.  Nothing the chain computes reads `t`.  The proposal's lane is read ahead of the predicate, with every lane active, as the
// body reads it for rset: inside `if (keep)` lane k would be inactive, and a value reloaded from scratch there is lane 0's only.
#define MCSAS_WIDE_KERNEL chain_wide_trace_kernel
#define MCSAS_WIDE_TRACE_PARAM , const TraceArgs t
#define MCSAS_WIDE_TRACE_START(c) if (tid == 0) t.chisq0[rep] = c;
#define MCSAS_WIDE_TRACE_MOVE(i, s, c, k)                                                                              \
    {                                                                                                                  \
        const bool keep = tid == 0 && i < (int64_t)t.capacity;                                                         \
        const size_t rec = (size_t)rep * (size_t)t.capacity + (size_t)i;                                               \
        _Pragma("unroll") for (int p = 0; p < MCSAS_MAX_ACTIVE; ++p)                                                   \
            if (p < P) {                                                                                               \
                const double tv = readlane_f64(prow[p], k);                                                            \
                if (keep) t.values[rec * P + p] = tv;                                                                  \
            }                                                                                                          \
        if (keep) { t.step[rec] = s; t.chisq[rec] = c; }                                                               \
    }
#include "chain_wide.h"
#undef MCSAS_WIDE_KERNEL
#undef MCSAS_WIDE_TRACE_PARAM
#undef MCSAS_WIDE_TRACE_START
#undef MCSAS_WIDE_TRACE_MOVE
#undef MCSAS_WIDE_PASS

#endif  // MCSAS_CHAIN_WIDE_H
#else   // MCSAS_WIDE_PASS: one kernel of the family
namespace mcsas {

// GIVEN: the chain is started from a given set (mcsas_hip_plan_set_start): the host has copied the repetition's start into rset
// ahead of the launch, and the first attempt takes it where the cold kernel generates one (chain_body.inc: GIVEN).  Here several waves
// run that branch.  In the first attempt every wave reads rset[n * P + p] while wave 0 (CHAIN_FIRST) stores what it has just read back
// to the same address: the same 8-byte value, bit for bit, in one aligned store, so a reader gets that value whichever side of the
// store it lands on.  No other access to rset crosses a wave boundary without a barrier: an accepted row is written by thread 0 and
// read by nobody during the attempt (the row cache is always on), and the fresh set of a retry is written by wave 0, which reaches
// it only through the barriers of the attempt before (the sums of its initial and final fits), behind every wave's last read of the
// start; nobody reads that set back.
template <int M, int QPL, bool GIVEN>
__global__ __launch_bounds__(WIDE_MAX_WAVES * 64) void MCSAS_WIDE_KERNEL(const ChainArgs a, const double *q3inv_glb MCSAS_WIDE_TRACE_PARAM) {
    extern __shared__ double lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, NW = blockDim.x >> 6;
    const int rep = blockIdx.x;
    const int N = a.n_contrib, P = a.model.n_active, qpad = a.qpad;
    const int q0 = wave * QPL * WAVE;                              // first q index of this wave's slice
    double *part = lds, *tab = lds + WIDE_PART_DOUBLES;
    int32_t *stop_word = reinterpret_cast<int32_t *>(part + 2 * WIDE_MAX_WAVES * 4);
    // the model's tables and the per-wave row scratch (make_qtables finds the latter behind the former)
    int tabd = Contrib<M>::table_doubles(a.model.int_div);
    if constexpr (Contrib<M>::ROWTAB > 0) { if (a.model.use_rowtab) tabd += NW * Contrib<M>::ROWTAB * a.model.int_div; }
    const double *qsrc = a.q, *q3src = q3inv_glb;
    if (a.pad1) {                                                  // q and 1/q^3 fit in LDS
        double *lq = tab + tabd, *lq3 = lq + qpad;
        for (int i = tid; i < qpad; i += blockDim.x) { lq[i] = a.q[i]; lq3[i] = q3inv_glb[i]; }
        qsrc = lq; q3src = lq3;
    }
    Contrib<M>::fill_table(a.model, tab, tid, blockDim.x);
    if (tid == 0) *stop_word = 0;
    __syncthreads();
    QTables qt = make_qtables<M>(a.model, qsrc + q0, q3src + q0, tab);
    if (qt.locs_t) qt.locs_t += q0;                                // smearing: evaluation points of this slice
    double lw[QPL], lwI[QPL];
#pragma unroll
    for (int j = 0; j < QPL; ++j) { lw[j] = a.w[q0 + lane + WAVE * j]; lwI[j] = a.wI[q0 + lane + WAVE * j]; }

    // the chain itself is chain_wave.h's (chain_body.inc), with a wave's slice of the q-points: the slice's column folded into the
    // cache pointer, w and wI from the registers above, sums over the workgroup and the row cache always on
    constexpr bool CACHE = true;
#define CHAIN_STATE int par = 0;
#define CHAIN_CACHE_PTR(p) (p + q0 + lane)
#define CHAIN_ROW(r) (size_t)(r) * qpad
#define CHAIN_Q(j) q0 + lane + WAVE * j
#define CHAIN_W(j) lw[j]
#define CHAIN_WI(j) lwI[j]
#define CHAIN_SUM3(x, y, z) wide_sum3(x, y, z, part, par, wave, lane, NW)
#define CHAIN_SUM1(x) wide_sum1(x, part, par, wave, lane, NW)
#define CHAIN_FIRST (wave == 0)
#define CHAIN_LEADER (tid == 0)
#define CHAIN_STOP wide_stop(a, stop_word, tid)
#define CHAIN_TRACE_START(c) MCSAS_WIDE_TRACE_START(c)
#define CHAIN_TRACE_MOVE(i, s, c, k) MCSAS_WIDE_TRACE_MOVE(i, s, c, k)
#include "chain_body.inc"
#undef CHAIN_STATE
#undef CHAIN_CACHE_PTR
#undef CHAIN_ROW
#undef CHAIN_Q
#undef CHAIN_W
#undef CHAIN_WI
#undef CHAIN_SUM3
#undef CHAIN_SUM1
#undef CHAIN_FIRST
#undef CHAIN_LEADER
#undef CHAIN_STOP
#undef CHAIN_TRACE_START
#undef CHAIN_TRACE_MOVE
}

}  // namespace mcsas
#endif  // MCSAS_WIDE_PASS
