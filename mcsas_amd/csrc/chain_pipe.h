// chain_pipe.h — the speculative proposal window of chain_wg.h spread over the WHOLE chip for runs
// with fewer chains than CUs (BASELINE config 2: 50 chains on 256 CUs).
//
// One launch per "tick" t (pipe_tick_kernel), two kinds of workgroup in its grid:
//   producer blocks (four per chain at config 2) do PROD(t+1): the form-factor rows of the NEXT window of Kb steps.
//       A block owns 8 * rows_per_wave consecutive steps = one or more SUB-WINDOWS of W steps: per step
//       d = new - old to the window buffer, the three ft-independent sums (a = Σ w d, e = Σ wI d, g = Σ w d²),
//       and — fp64 MFMA, v_mfma_f64_16x16x4_f64 — the sub-window's Gram block G[a][k] = Σ_q w d_a d_k, which does
//       not depend on ft either.  Rows without an integral: the sub-window's d rows stay in LDS for the MFMAs, no
//       `new` row is stored and a contribution's cached row is evaluated again when it has gone stale (lazy rows);
//       Rows with an integral (or a smeared model) — the kernel instantiation pipe_tick_kernel<M, QPL, true>: the producer waves
//       of a chain PULL the window's rows from a queue, most expensive first, blocks whose queue is empty join other chains'
//       (pipe_prod_rowq); `new` row into a spare HBM row slot, slots swapped on acceptance; the Gram blocks (8 steps) are taken by
//       the scan block from the rows it has in LDS.
//   scan blocks (one per chain) do SCAN(t): per sub-window ONE pass over its d rows gives h_k = Σ (w ft) d_k for
//       the ft the sub-window starts from (eight waves, rows streamed HBM/L2 -> registers); then ONE wave takes
//       the W decisions with lane g = step g: a candidate's fit sums are SC + a, SIC + e, SCC + 2h + g, and after
//       an accepted row `acc` the later steps of the sub-window need only h_k += G[acc][k] (one LDS read) — no
//       barrier, no re-reduction and no restart per accepted move; the accepted rows are applied to ft once per
//       sub-window, in order, as ft += d.
// PROD(t+1) and SCAN(t) run concurrently inside one launch because a window's rows depend only on the random
// stream and on row slots settled two windows earlier (2*Kb <= N), never on the decisions of the window
// before.  Launch t+1 follows launch t on the same stream: the kernel boundary is the only synchronisation
// between workgroups; there are no in-kernel spin waits and no cross-workgroup flags (the row queue's counters are
// fetch-and-add tickets: nobody waits on them).
//
// Chain schedule: an attempt (one mcFit call) is initialised at tick t_init (PROD evaluates the N
// rows of the initial set, SCAN sums them and fits), then tick t > t_init handles window
// t - t_init - 1.  SCAN(t) publishes the small schedule record PROD(t+2) reads, double-buffered by
// tick parity, so a producer never reads a record that a concurrently running scan is writing.
//
// Files: pipe_layout.h (argument blocks, constants, pipe_geometry: all the host needs), pipe_gram.h (Gram blocks of the producers),
// pipe_rowq.h (producers pulling rows from a queue), pipe_prod.h (producer block; pipe_prod_overlap.inc: its tuning-build variant),
// pipe_scan.h (scan block); the tick and reset kernels are here.
#pragma once
#include "pipe_layout.h"
#include "pipe_gram.h"
#include "pipe_rowq.h"
#include "pipe_prod.h"
#include "pipe_scan.h"

namespace mcsas {

// ------------------------------------------------------------------------------------ one tick
// launch t: blocks [0, R) do SCAN(t) (skipped for t < 0), the others PROD(t + 1)
template <int M, int QPL, bool RQ>
__global__ __launch_bounds__(PIPE_BLOCK) void pipe_tick_kernel(const PipeArgs *pap, const int tick, const int stop_now, const PipeHot hot) {
    // The argument block lives in device memory and is read where it is needed: passed by value it
    // would sit in SGPRs for the whole kernel (600+ bytes) and the scan loop would run on spilled
    // scalars (one v_readlane per use).
    extern __shared__ double lds[];
    const PipeArgs &pa = *pap;
    const int R = hot.n_reps, b = blockIdx.x, t = tick;
#ifdef MCSAS_STAMPS
    struct Timeline {                                          // one record per wave, written when the wave leaves the kernel
        uint64_t *p, t0; uint32_t hw;
        __device__ Timeline(const PipeArgs &pa, int tick) {
            p = (pa.timeline && tick == pa.timeline_tick && (threadIdx.x & 63) == 0) ? pa.timeline + ((size_t)blockIdx.x * 8 + (threadIdx.x >> 6)) * PIPE_TL_WORDS : nullptr;
            t0 = wall_clock64();
            hw = __builtin_amdgcn_s_getreg((4 << 0) | (0 << 6) | (31 << 11));   // HW_ID
        }
        __device__ ~Timeline() { if (p) { p[0] = t0; p[1] = wall_clock64(); p[2] = hw; p[3] = __builtin_amdgcn_s_getreg((20 << 0) | (0 << 6) | (31 << 11)); } }   // XCC_ID
    } timeline_record(pa, tick);
#endif
    if (b < R) {
        if (t >= 0) {
            // rows per wave and sub-window: uniform for the launch; the host only picks combinations instantiated here
            if constexpr (RQ) pipe_scan_block<M, QPL, 1, true>(pa, lds, b, t, stop_now);       // (sub-windows of 8 steps)
            else switch (hot.w_sub >> 3) {
#define PIPE_SCAN_CASE(r) case r: if constexpr (r * QPL <= PIPE_MAX_ROW_DOUBLES) pipe_scan_block<M, QPL, r, false>(pa, lds, b, t, stop_now); break;
                PIPE_SCAN_CASE(1) PIPE_SCAN_CASE(2) PIPE_SCAN_CASE(3) PIPE_SCAN_CASE(4) PIPE_SCAN_CASE(6) PIPE_SCAN_CASE(8)
#undef PIPE_SCAN_CASE
                default: break;
            }
        }
    } else {
        // chain-major block -> (chain, sub-window) map: round-robin dispatch then spreads every chain's blocks
        // over the 8 XCDs.  The XCD-aware alternative (diagnostic bit 128: chain r's producer blocks on block ids
        // congruent to r modulo 8, i.e. on the XCD of its scan block, so that next tick's d rows sit in that
        // XCD's L2) measured 10-40 % SLOWER on config 2: 50 chains x (1 + gy) blocks do not divide over 8 XCDs of
        // 32 CUs with one block per CU — two XCDs get 35 blocks and their chains take two rounds.
        const int gy = hot.prod_blocks_y;
        int rep = (b - R) / gy, y = (b - R) % gy;
        // rows pulled from a queue: block-major over the chains (b = R + y R + rep), so that the workgroups that have to wait for a
        // CU — the launch has more of them than the chip — are the LAST block of every chain, not all blocks of the last chains
        if constexpr (RQ) { rep = (b - R) % R; y = (b - R) / R; }
        if (MCSAS_TUNE_BITS(pa.c) & 128) { const int x = b & 7, j = (b - R) >> 3; rep = x + 8 * (j / gy); y = j % gy; }
        if (rep < R) pipe_prod_block<M, QPL, RQ>(pa, hot, lds, rep, y, gy, t + 1);
    }
}

// first tick bookkeeping: schedule records for ticks 0 and 1, counters
template <int UNUSED>
__global__ void pipe_reset_kernel(const PipeArgs *pap) {
    const PipeArgs &pa = *pap;
    const int rep = blockIdx.x * blockDim.x + threadIdx.x;
    if (rep >= pa.c.n_reps) return;
    const ChainArgs &a = pa.c;
    PipeChain ch{};
    PipeSnap s{};
    s.attempt = 0; s.t_init = 0; s.alive = 1;
    s.init_base = 0;
    s.step_base = MCSAS_INITIAL_DRAWS(a, a.n_contrib, a.model.n_active);
    ch.snap[0] = s; ch.snap[1] = s;
    ch.attempts = 1; ch.chi2 = 0.; ch.A = 1.; ch.t_start = wall_clock64();
    pa.chains[rep] = ch;
    if (pa.rowq) { pa.rowq[(size_t)rep * 2] = 0; pa.rowq[(size_t)rep * 2 + 1] = 0; }
}

}  // namespace mcsas
