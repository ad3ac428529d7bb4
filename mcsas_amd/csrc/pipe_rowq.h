// pipe_rowq.h — producer blocks of the pipeline (chain_pipe.h) for rows with an integral: the waves of a chain pull the
// window's rows from a queue, and a block whose queue is empty helps another chain.
#pragma once
#include "pipe_gram.h"      // PIPE_LDS_BARRIER

namespace mcsas {

// schedule records go through scalar global loads / stores (a struct copy out of an address-space-qualified
// reference does not exist in C++)
__device__ __forceinline__ PipeSnap load_snap(const PipeSnap *p) {
    PipeSnap s;
    s.attempt = glb(&p->attempt)[0]; s.t_init = glb(&p->t_init)[0]; s.alive = glb(&p->alive)[0]; s.pad = 0;
    s.init_base = glb(&p->init_base)[0]; s.step_base = glb(&p->step_base)[0];
    return s;
}
__device__ __forceinline__ void store_snap(PipeSnap *p, const PipeSnap &s) {
    glb(&p->attempt)[0] = s.attempt; glb(&p->t_init)[0] = s.t_init; glb(&p->alive)[0] = s.alive; glb(&p->pad)[0] = 0;
    glb(&p->init_base)[0] = s.init_base; glb(&p->step_base)[0] = s.step_base;
}

// ------------------------------------------------------------------------------------ producer, rows with an integral
// Rows of these models (or of a smeared one) cost 10^4 .. 10^5 instructions and up to five times their neighbour's (a worm's Kuhn
// length sets the number of quadrature panels, a cylinder's radius the Bessel function's branch): with a static deal a tick lasted as
// long as its unluckiest wave (13 worm chains: 0.47 of the issue rate; 256 chains, whose many blocks the dispatcher balances: 0.70).
// The producer waves of a chain PULL rows instead, from a counter per chain and tick parity in device memory (PipeArgs::rowq, zeroed a
// tick ahead by the scan block):
//   window tick  1. the block works out the proposals of ALL Kb steps of the window, one per thread (draw, generator transform,
//                   prepare(), predicted cost: models.h row_cost), and parks the records in LDS — 500 instructions per step against
//                   10^5 for its row;
//                2. every thread ranks its step by predicted cost (most expensive first; steps behind max_iter last);
//                3. every wave takes the next rank from the counter until the window is handed out: longest rows first, the short
//                   ones fill the gaps.
//   initial tick the contributions of the initial set, four at a time.
// No Gram phase here: the scan block has the rows of an 8-step sub-window in its LDS anyway and takes the 28 dot products there
// (pipe_scan_block) — the steps of a sub-window are no longer evaluated by one workgroup.
// One visit = one chain's queue worked on until it is empty.  `helper`: the chain is not the block's own (pipe_prod_rowq).
template <int M, int QPL>
__device__ __forceinline__ void pipe_rowq_visit(const PipeArgs &pa, const PipeHot &hot, double *lds, const QTables &qt, int rep, int by, int gy, int t,
                                                const PipeSnap &sn, bool helper) {
    const ChainArgs &a = pa.c;
    const int tid = threadIdx.x, lane = tid & 63;
    const int N = hot.n_contrib, P = hot.n_active, qpad = hot.qpad, Kb = hot.kb;
    const int64_t max_iter = hot.max_iter;
    double *lq = lds, *lw = lds + qpad, *lwI = lds + 2 * qpad;
    auto rset = glb(a.rset) + (size_t)rep * N * P;
    auto cache = glb(a.cache) + (size_t)rep * a.cache_rows * qpad;
    const DrawSource src MCSAS_CHAIN_DRAWS(a, rep);
    auto slot_of = glb(pa.slot_of) + (size_t)rep * N;
    auto stage = glb(pa.stage_slot) + (size_t)rep * 2 * Kb;
    auto row_valid = glb(pa.row_valid) + (size_t)rep * N;
    int32_t *rowq = pa.rowq + (size_t)rep * 2 + (t & 1);

    if (t == sn.t_init) {
        // ---- initial parameter set of the attempt (mcsas.py:310-319).  (A static share per wave would make the workgroups that
        // wait for a CU — the launch has more of them than the chip — a second round as long as the first.)
        if (!helper) {
            for (int i = tid + by * PIPE_BLOCK; i < N; i += PIPE_BLOCK * gy) { slot_of[i] = i; row_valid[i] = 1; }
            for (int i = tid + by * PIPE_BLOCK; i < 2 * Kb; i += PIPE_BLOCK * gy) stage[i] = N + i;
        }
        int ovf = 0;
        constexpr int CH = 4;
        for (int pulls = 0; pulls * CH <= N; ++pulls) {
            int n0 = 0;
            if (lane == 0) n0 = __hip_atomic_fetch_add(rowq, CH, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            n0 = __builtin_amdgcn_readfirstlane(n0);
            if (n0 < 0 || n0 >= N) break;
            const int n = n0 + lane;
            double row[MCSAS_MAX_ACTIVE] = {0., 0., 0., 0.};
            MCSAS_INITIAL_ROW(row, n, lane < CH && n < N, false, true, sn.init_base, ovf)
            Contrib<M> mine;
            mine.prepare(a.model, row);
            for (int l = 0; l < CH && n0 + l < N; ++l) {
                const Contrib<M> c = mine.bcast(__builtin_amdgcn_readfirstlane(l));
                double it[QPL];
                RowEval<M, QPL>::run(c, qt, lane, it);
#pragma unroll
                for (int j = 0; j < QPL; ++j) cache[(size_t)(n0 + l) * qpad + lane + WAVE * j] = it[j];
            }
        }
        if (__any(ovf) && lane == 0) atomicOr(&pa.chains[rep].overflow, 1);
        return;
    }

    // ---- window w of the attempt
    const int64_t w = (int64_t)t - sn.t_init - 1;
    const int buf = t & 1;
    const int64_t s0 = w * Kb;
    const int64_t left = max_iter - s0;
    const int nvalid = left >= Kb ? Kb : (left > 0 ? (int)left : 0);
    constexpr int CON = (int)(sizeof(Contrib<M>) / 8), REC = CON + MCSAS_MAX_ACTIVE + 2;   // Contrib | proposal values | overflow flag | cost
    static_assert(sizeof(Contrib<M>) % 8 == 0, "Contrib record");
    double *rec = lds + pa.g.rec_off;                         // [Kb][REC]
    int32_t *order = reinterpret_cast<int32_t *>(rec + (size_t)Kb * REC);   // [Kb] rank -> step of the window
    int32_t *rslot = order + Kb;                              // [Kb][2] row slot of the step's contribution, spare slot for its new row
    for (int k = tid; k < Kb; k += PIPE_BLOCK) {
        double prow[MCSAS_MAX_ACTIVE] = {0., 0., 0., 0.};
        int pov = 0;
        MCSAS_PROPOSAL_ROW(prow, sn.step_base + (uint64_t)(s0 + k) * P, k < nvalid, pov)
        Contrib<M> prop;
        prop.prepare(a.model, prow);
        double cost = -1.0;                                   // (steps behind max_iter: last)
        if (k < nvalid) cost = Contrib<M>::ROW_CLASS == 2 ? row_cost<M, QPL>(prop, lq) : 0.0;
        double tmp[CON];
        __builtin_memcpy(tmp, &prop, sizeof(Contrib<M>));
#pragma unroll
        for (int i = 0; i < CON; ++i) rec[(size_t)k * REC + i] = tmp[i];
#pragma unroll
        for (int p = 0; p < MCSAS_MAX_ACTIVE; ++p) rec[(size_t)k * REC + CON + p] = prow[p];
        rec[(size_t)k * REC + CON + MCSAS_MAX_ACTIVE] = (double)pov;
        rec[(size_t)k * REC + CON + MCSAS_MAX_ACTIVE + 1] = cost;
        const int r = (int)((s0 + k) % N);
        rslot[2 * k] = slot_of[r]; rslot[2 * k + 1] = stage[buf * Kb + k];
    }
    __syncthreads();
    for (int k = tid; k < Kb; k += PIPE_BLOCK) {
        int rank = k;
        if constexpr (Contrib<M>::ROW_CLASS == 2) {
            const double cst = rec[(size_t)k * REC + CON + MCSAS_MAX_ACTIVE + 1];
            rank = 0;
            for (int j = 0; j < Kb; ++j) {
                const double cj = rec[(size_t)j * REC + CON + MCSAS_MAX_ACTIVE + 1];
                rank += (cj > cst || (cj == cst && j < k)) ? 1 : 0;
            }
        }
        order[rank] = k;
    }
    PIPE_LDS_BARRIER();
    auto dwin = glb(pa.dwin) + ((size_t)rep * 2 + buf) * Kb * qpad;
    auto scal = glb(pa.scal) + ((size_t)rep * 2 + buf) * Kb * 4;
    auto pval = glb(pa.pval) + ((size_t)rep * 2 + buf) * Kb * MCSAS_MAX_ACTIVE;
    auto povf = glb(pa.povf) + ((size_t)rep * 2 + buf) * Kb;
    if (MCSAS_TUNE_BITS(a) & 16) return;                                  // diagnostic: no window rows
    for (int pulls = 0; pulls <= Kb; ++pulls) {               // (a wave can draw at most every row of the window: the loop ends whatever the counter holds)
        int idx = 0;
        if (lane == 0) idx = __hip_atomic_fetch_add(rowq, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        idx = __builtin_amdgcn_readfirstlane(idx);
        if (idx < 0 || idx >= nvalid) break;                  // (the ranks behind nvalid are the steps behind max_iter)
        const int k = __builtin_amdgcn_readfirstlane(order[idx]);
        Contrib<M> cnew;
        {
            double tmp[CON];
#pragma unroll
            for (int i = 0; i < CON; ++i) tmp[i] = readlane_f64(rec[(size_t)k * REC + i], 0);   // one address for the wave: into scalar registers
            __builtin_memcpy(&cnew, tmp, sizeof(Contrib<M>));
        }
        const int oslot = __builtin_amdgcn_readfirstlane(rslot[2 * k]), sslot = __builtin_amdgcn_readfirstlane(rslot[2 * k + 1]);
        const auto nrow = cache + (size_t)sslot * qpad + lane;
        const auto dr = dwin + (size_t)k * qpad + lane;
        // d = new - old and the three sums that do not depend on ft: a = Σ w d, e = Σ wI d, g = Σ w d².  Every q slot is
        // consumed the moment the evaluator has it (RowEval::run_each) and nothing of the row stays in registers across the
        // evaluation of the next slot (the row arrays used to be spilled to scratch around every slot: 20-30 KB per step); the
        // `old` value of a slot is requested one slot ahead and lands while that slot is evaluated.
        const auto orow = cache + (size_t)oslot * qpad + lane;
        double s1 = 0., s2 = 0., s3 = 0.;
        double o_ahead = orow[0];
        RowEval<M, QPL>::run_each(cnew, qt, lane, [&](int j, double v) {
            const int iq = lane + WAVE * j;
            const double o = o_ahead;
            o_ahead = orow[WAVE * (j + 1 < QPL ? j + 1 : j)];
            nrow[WAVE * j] = v;
            const double dj = v - o;
            dr[WAVE * j] = dj;
            const double wd = lw[iq] * dj;
            s1 += wd; s2 = fma(lwI[iq], dj, s2); s3 = fma(wd, dj, s3);
        });
        wave_sum3(s1, s2, s3);
        if (lane == 0) { scal[k * 4 + 0] = s1; scal[k * 4 + 1] = s2; scal[k * 4 + 2] = s3; }
        if (lane < P) pval[k * MCSAS_MAX_ACTIVE + lane] = rec[(size_t)k * REC + CON + lane];
        if (lane == 0) povf[k] = (int)rec[(size_t)k * REC + CON + MCSAS_MAX_ACTIVE];
    }
}

// The block's own chain first; then it HELPS.  The launch holds more producer workgroups than the chip has CUs (so that the CUs the
// scan blocks leave after a tenth of a tick are taken over), the chains do not get their workgroups at the same time, and chains that
// have converged — or wait for their next attempt — need none: a block whose queue is empty looks at what is left in EVERY chain's
// queue (one chain per thread: schedule record and counter), and joins one picked with probability proportional to the rows left
// (by a hash of the block index, so that the helpers spread like the work) if that is worth the 500 instructions per step of working
// out that chain's proposals again.  The tick then ends when the rows of ALL chains are done, and the last chains of an analysis that
// runs to its criterion get the whole chip.  Bounded: PIPE_HELP_TRIES visits per block, none once every queue is (nearly) empty.
constexpr int PIPE_HELP_TRIES = 8;
constexpr int PIPE_HELP_MIN_ROWS = 4;
template <int M, int QPL>
__device__ __forceinline__ void pipe_prod_rowq(const PipeArgs &pa, const PipeHot &hot, double *lds, const QTables &qt, int rep, int by, int gy, int t,
                                               const PipeSnap &sn, bool own) {
    const int tid = threadIdx.x, lane = tid & 63, R = hot.n_reps, N = hot.n_contrib, Kb = hot.kb;
    if (own) pipe_rowq_visit<M, QPL>(pa, hot, lds, qt, rep, by, gy, t, sn, false);
    if (!pa.g.help) return;
    int32_t *box = reinterpret_cast<int32_t *>(lds + pa.g.gram_off);       // (the 16 doubles ahead of the proposal records)
    int32_t *rem = reinterpret_cast<int32_t *>(lds + pa.g.rec_off);        // [R] rows left per chain (the records' place: pipe_geometry sets `help` only if they fit)
    for (int tries = 0; tries < PIPE_HELP_TRIES; ++tries) {
        __syncthreads();                                          // every wave is done with the records of the last visit
        for (int c = tid; c < R; c += PIPE_BLOCK) {
            int r = 0;
            const PipeSnap cs = load_snap(&hot.chains[c].snap[t & 1]);
            if (cs.alive && t >= cs.t_init) {
                int total = N;
                if (t > cs.t_init) {
                    const int64_t left = hot.max_iter - ((int64_t)t - cs.t_init - 1) * Kb;
                    total = left >= Kb ? Kb : (left > 0 ? (int)left : 0);
                }
                r = total - __hip_atomic_load(pa.rowq + (size_t)c * 2 + (t & 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (r < PIPE_HELP_MIN_ROWS) r = 0;
            }
            rem[c] = r;
        }
        __syncthreads();
        if (tid < 64) {
            const int chunk = (R + 63) / 64, lo = lane * chunk, hi = min(R, lo + chunk);
            int sum = 0;
            for (int c = lo; c < hi; ++c) sum += rem[c];
            int incl = sum;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_up(incl, d); if (lane >= d) incl += o; }
            const int total = __builtin_amdgcn_readlane(incl, 63);
            if (lane == 0) box[0] = -1;
            if (total > 0) {
                const uint32_t hsh = ((uint32_t)blockIdx.x * 2654435761u) ^ ((uint32_t)(tries + 1) * 0x9E3779B9u) ^ ((uint32_t)t * 0x85EBCA6Bu);
                const int pos = (int)((hsh >> 8) % (uint32_t)total);
                if (pos >= incl - sum && pos < incl) {            // exactly one lane
                    int acc = incl - sum, pick = lo;
                    for (int c = lo; c < hi; ++c) { if (pos < acc + rem[c]) { pick = c; break; } acc += rem[c]; }
                    box[0] = pick;
                }
            }
        }
        __syncthreads();
        const int target = box[0];
        if (target < 0) break;
        const PipeSnap cs = load_snap(&hot.chains[target].snap[t & 1]);
        pipe_rowq_visit<M, QPL>(pa, hot, lds, qt, target, by, gy, t, cs, true);
    }
}

}  // namespace mcsas
