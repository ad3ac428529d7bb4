// chain_wave_kernel.inc — what the four wave-per-chain kernels of chain_wave.h do once they know their analysis: the block's LDS
// tables, then the chain (chain_body.inc) with the q-points of a wave: q index lane + 64 j in slot j, w and wI read from LDS, sums
// by DPP inside the wave, every lane a first-wave lane and lane 0 the leader.  Included verbatim so that all four compile from the
// same text.  In scope at the point of inclusion: M, QPL, CACHE (template parameters), GIVEN (compile-time bool),
// `const ChainArgs &a`, `const int rep`, `lds` (the dynamic LDS), `const int lane` — and the two macros MCSAS_WAVE_TRACE_START /
// MCSAS_WAVE_TRACE_MOVE, which stand for nothing except in the traced kernel (chain_wave.h sets them).
    const int N = a.n_contrib, P = a.model.n_active, qpad = a.qpad;
    double *lq = lds, *lw = lds + qpad, *lwI = lds + 2 * qpad, *lq3 = lds + 3 * qpad, *tab = lds + 4 * qpad;
    for (int i = lane; i < qpad; i += WAVE) {
        const double qq = a.q[i];
        lq[i] = qq; lw[i] = a.w[i]; lwI[i] = a.wI[i]; lq3[i] = 1.0 / (qq * qq * qq);
    }
    const QTables qt = make_qtables<M>(a.model, lq, lq3, tab);
    Contrib<M>::fill_table(a.model, tab, lane, WAVE);
    __syncthreads();

#define CHAIN_STATE
#define CHAIN_CACHE_PTR(p) p
#define CHAIN_ROW(r) (size_t)(r) * qpad + lane
#define CHAIN_Q(j) lane + WAVE * j
#define CHAIN_W(j) lw[lane + WAVE * j]
#define CHAIN_WI(j) lwI[lane + WAVE * j]
#define CHAIN_SUM3(x, y, z) wave_sum3(x, y, z)
#define CHAIN_SUM1(x) wave_sum(x)
#define CHAIN_FIRST true
#define CHAIN_LEADER (lane == 0)
#define CHAIN_STOP stop_requested(a)                        // (one answer per wave: chain_common.h)
#define CHAIN_TRACE_START(c) MCSAS_WAVE_TRACE_START(c)
#define CHAIN_TRACE_MOVE(i, s, c, k) MCSAS_WAVE_TRACE_MOVE(i, s, c, k)
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
