// pipe_prod.h — producer block of the pipeline (chain_pipe.h): start-up, the initial parameter set, and for rows without an
// integral the window's rows sub-window by sub-window with their Gram blocks (pipe_gram.h); rows with an integral go to
// pipe_rowq.h.  A tuning build includes the overlapped variant of the row loop, pipe_prod_overlap.inc, in place.
#pragma once
#include "pipe_rowq.h"
#include <type_traits>

namespace mcsas {

// Producer row loop: the memory counter of gfx950 is in order over loads AND stores, so a wait for the `old` row of the
// next step that comes behind this step's sixteen row stores drains them (a memory round trip per row).  The rows are
// therefore waited for HERE, in front of the stores: everything outstanding at this point was issued before the row was
// evaluated.  Routing the values through an empty asm pins the wait (and the stores behind it) to this place.
#define PIPE_PIN_ROW(arr) do { _Pragma("unroll") for (int j_ = 0; j_ < QPL; ++j_) asm volatile("" : "+v"(arr[j_])); } while (0)

// Stamps build (-DMCSAS_STAMPS): marks of tick `timeline_tick` in the timeline record of a wave (PIPE_TL_WORDS)
#ifdef MCSAS_STAMPS
#define PIPE_TL_SLOT(pa, i) (pa).timeline[((size_t)blockIdx.x * 8 + (threadIdx.x >> 6)) * PIPE_TL_WORDS + 4 + (i)]
#define PIPE_TL_PUT(pa, t, i, val) do { if ((pa).timeline && (t) - 1 == (pa).timeline_tick && (threadIdx.x & 63) == 0) PIPE_TL_SLOT(pa, i) = (val); } while (0)
#define PIPE_TL_CLOCK(var) const uint64_t var = wall_clock64()   /* entry marks 22..25: clocks taken into registers (no argument-block read in the way), written later */
#else
#define PIPE_TL_PUT(pa, t, i, val) do {} while (0)
#define PIPE_TL_CLOCK(var) do {} while (0)
#endif
#define PIPE_TL_WRITE(pa, t, i) PIPE_TL_PUT(pa, t, i, wall_clock64())
#define PIPE_TLX_MARK(pa, t, i) PIPE_TL_WRITE(pa, t, 18 + (i))   /* start-up marks 18..21: tables in LDS, proposals prepared, stale rows refreshed, row loop */
#define PIPE_TL_MARK(pa, t, i) PIPE_TL_WRITE(pa, t, i)

// Models whose row costs a few hundred instructions (no orientation / contour integral): their producers store no `new`
// rows (4 KB per step) — a contribution's cached row goes stale when its proposal is accepted and is evaluated again,
// one q per thread, by the producer block that needs it as `old` N steps later (PipeGeom::lazy_rows).
// Same function, same inputs as RowEval -> the same bits.
// (Contrib<M>::ROW_CLASS == 0: sphere, core-shell sphere, Gaussian chain, LMA dense spheres)
template <int M> constexpr bool pipe_light_model_v = Contrib<M>::ROW_CLASS == 0;
template <int M>
__device__ __forceinline__ double pipe_point_intensity(const Contrib<M> &c, double q, double q3inv, const double *tab) {
    if constexpr (M == MCSAS_MODEL_SPHERE) return c.fast ? c.intensity_fast(q, q3inv) : c.intensity(q, tab);
    else return c.intensity(q, tab);
}

// one row of the window buffers as every kernel here holds it in registers: 16-byte loads, lane l and
// register pair c <-> q = 128 c + 2 l + {0, 1}  (QPL = 1: one 8-byte load, q = l)
template <int QPL>
__device__ __forceinline__ void load_row_pairs(const MCSAS_GLOBAL double *row, int lane, double (&r)[QPL]) {
    if constexpr (QPL >= 2) {
#pragma unroll
        for (int c = 0; c < QPL / 2; ++c) {
            const v2f64 v = *(const MCSAS_GLOBAL v2f64 *)(row + 128 * c + 2 * lane);
            r[2 * c] = v.x; r[2 * c + 1] = v.y;
        }
    } else {
        r[0] = row[lane];
    }
}
template <int QPL>
__device__ __forceinline__ void load_row_pairs_lds(const double *row, int lane, double (&r)[QPL]) {
    if constexpr (QPL >= 2) {
#pragma unroll
        for (int c = 0; c < QPL / 2; ++c) {
            const v2f64 v = *reinterpret_cast<const v2f64 *>(row + 128 * c + 2 * lane);
            r[2 * c] = v.x; r[2 * c + 1] = v.y;
        }
    } else {
        r[0] = row[lane];
    }
}

template <int M, int QPL, bool RQ>                            // RQ: rows pulled from a queue (PipeGeom::rowq), a kernel of its own
__device__ __forceinline__ void pipe_prod_block(const PipeArgs &pa, const PipeHot &hot, double *lds, int rep, int by, int gy, int t) {
    const ChainArgs &a = pa.c;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr int WPB = PIPE_BLOCK / 64;
    const int N = hot.n_contrib, P = hot.n_active, qpad = hot.qpad, Kb = hot.kb;
    const int64_t max_iter = hot.max_iter;                    // (a field of the argument block read inside the row loop would be a global load + full wait per row)
    // the data tables do not depend on the chain's schedule record: both round trips run side by side
    constexpr int QTB = (QPL * 64 + PIPE_BLOCK - 1) / PIPE_BLOCK;
    double tq[QTB], tw[QTB], twI[QTB], tq3[QTB];
#pragma unroll
    for (int x = 0; x < QTB; ++x) {
        const int i = tid + PIPE_BLOCK * x < qpad ? tid + PIPE_BLOCK * x : 0;
        tq[x] = glb(hot.q)[i]; tw[x] = glb(hot.w)[i]; twI[x] = glb(hot.wI)[i]; tq3[x] = glb(hot.q3inv)[i];
    }
    PIPE_TL_CLOCK(c_entry);                                   // (hot arguments in registers, loads issued)
    const PipeSnap sn = load_snap(&hot.chains[rep].snap[t & 1]);
    const bool own = sn.alive && t >= sn.t_init;
    if (!own && !(RQ && pa.g.help)) return;                   // (row queues: a block whose chain has nothing to do this tick helps the others)
    PIPE_TL_CLOCK(c_snap);

    double *lq = lds, *lw = lds + qpad, *lwI = lds + 2 * qpad, *lq3 = lds + 3 * qpad, *tab = lds + 4 * qpad;
#pragma unroll
    for (int x = 0; x < QTB; ++x) {
        const int i = tid + PIPE_BLOCK * x;
        if (i < qpad) { lq[i] = tq[x]; lw[i] = tw[x]; lwI[i] = twI[x]; lq3[i] = tq3[x]; }
    }
    PIPE_TL_CLOCK(c_tab);
    Contrib<M>::fill_table(a.model, tab, tid, PIPE_BLOCK);
    if (tid == 0) *reinterpret_cast<int32_t *>(lds + pa.g.gram_off + 16) = 0;   // lazy rows: the block's stale-row count
    __syncthreads();
    PIPE_TL_CLOCK(c_bar);
    PIPE_TL_PUT(pa, t, 22, c_entry); PIPE_TL_PUT(pa, t, 23, c_snap); PIPE_TL_PUT(pa, t, 24, c_tab); PIPE_TL_PUT(pa, t, 25, c_bar);
    const QTables qt = make_qtables<M>(a.model, lq, lq3, tab);
    if constexpr (RQ) { pipe_prod_rowq<M, QPL>(pa, hot, lds, qt, rep, by, gy, t, sn, own); return; }
    auto rset = glb(a.rset) + (size_t)rep * N * P;
    auto cache = glb(a.cache) + (size_t)rep * a.cache_rows * qpad;
    const DrawSource src{a.replay ? a.replay + (size_t)rep * a.replay_len : nullptr, a.replay_len, a.seed,
                         (uint32_t)(a.rep_offset + rep)};
    auto slot_of = glb(pa.slot_of) + (size_t)rep * N;
    auto stage = glb(pa.stage_slot) + (size_t)rep * 2 * Kb;
    auto row_valid = glb(pa.row_valid) + (size_t)rep * N;
    const int gw = by * WPB + wave, nw = gy * WPB;          // this wave's index among the chain's producer waves

    if (t == sn.t_init) {
        // ---- initial parameter set of the attempt (mcsas.py:310-319): rows n = gw*64 + lane + 64*nw*i
        for (int i = tid + by * PIPE_BLOCK; i < N; i += PIPE_BLOCK * gy) { slot_of[i] = i; row_valid[i] = 1; }
        for (int i = tid + by * PIPE_BLOCK; i < 2 * Kb; i += PIPE_BLOCK * gy) stage[i] = N + i;
        int ovf = 0;
        // contribution n = lane*nw + gw + 64*nw*i: every producer wave of the chain owns ~N/nw rows
        for (int nb = 0; nb < N; nb += nw * WAVE) {
            const int n = nb + lane * nw + gw;
            double row[MCSAS_MAX_ACTIVE] = {0., 0., 0., 0.};
            if (n < N) {
#pragma unroll
                for (int p = 0; p < MCSAS_MAX_ACTIVE; ++p)
                    if (p < P) {
                        if (a.start_from_min) row[p] = a.start_value[p];
                        else {
                            double u = src.at(sn.init_base + (uint64_t)p * N + n, ovf);
                            row[p] = gen_transform(a.gen_kind[p], u) * (a.gen_hi[p] - a.gen_lo[p]) + a.gen_lo[p];
                        }
                        rset[(size_t)n * P + p] = row[p];
                    }
            } else {
#pragma unroll
                for (int p = 0; p < MCSAS_MAX_ACTIVE; ++p) row[p] = a.gen_lo[p] > 0. ? a.gen_lo[p] : 1e-9;
            }
            Contrib<M> mine;
            mine.prepare(a.model, row);
            for (int l = 0; l < WAVE; ++l) {
                const int nn = nb + l * nw + gw;
                if (nn >= N) break;
                const Contrib<M> c = mine.bcast(__builtin_amdgcn_readfirstlane(l));
                double it[QPL];
                RowEval<M, QPL>::run(c, qt, lane, it);
#pragma unroll
                for (int j = 0; j < QPL; ++j) cache[(size_t)nn * qpad + lane + WAVE * j] = it[j];
            }
        }
        if (__any(ovf) && lane == 0) atomicOr(&pa.chains[rep].overflow, 1);
        return;
    }

    if (MCSAS_TUNE_BITS(a) & 16) return;                                  // diagnostic: no window rows
    if constexpr (pipe_light_model_v<M>) if (pa.g.overlap || pa.g.gram_lds) {   // (rows with an integral never take this path: not instantiated for them)
        // ---- overlapped producer.  The block's rows are nsb sub-windows of W; phase ss = the rows of sub-window ss, every
        // wave its share, d = new - old straight to the window buffer.  The Gram block of sub-window ss - 1 is worked off
        // in units BETWEEN the rows of phase ss (matrix pipe beside the vector pipe: while one wave of a SIMD is inside a run
        // of MFMAs its partner has the vector issue slots to itself), its operands read back from the window buffer.
        // One barrier per phase, and it waits for no memory: a wave passes B(ss - 1) — "the rows of ss - 1 are visible to the
        // workgroup" — behind its FIRST row of phase ss, after a counted wait that covers exactly its stores of phase
        // ss - 1 (the counter is in order: everything older than that row's own stores has completed by then).  The partial
        // tiles of a block are parked in LDS when a wave has done its last unit and summed by all threads behind the next
        // barrier (two reduction buffers, by parity).  Only the last sub-window's Gram block runs with nothing beside it.
        const int W = pa.g.w, nsb = pa.g.sub_per_block, BR = nsb * W;
        // Rows per wave and sub-window: W / 8 on average; tuning bits 19-20 shift rows from the four waves that share
        // their SIMDs with an older wave (4-7) to the older ones (0-3): 0 = equal shares, 1 / 2 = one / two rows.
        // (the LDS variant's default is one row: the SIMD arbitrates oldest-first, so with equal shares the older wave is done
        // early and the younger one finishes the phase alone, latency-bound — measured 4 + 2 rows 3.92 ms, 3 + 3 4.03, 5 + 1 4.2;
        // bits 19-20 = 3 there: equal shares)
        const int rw_even = W >> 3, skew_bits = (MCSAS_TUNE_BITS(a) >> 19) & 3;
        const int skew_req = pa.g.gram_lds ? (skew_bits == 0 ? 1 : (skew_bits == 3 ? 0 : skew_bits)) : skew_bits;
        const int skew = skew_req < rw_even ? skew_req : rw_even - 1;
        const int wv = __builtin_amdgcn_readfirstlane(wave);
        const int RW = wv < 4 ? rw_even + skew : rw_even - skew;                        // my rows per sub-window
        const int rbase = wv < 4 ? wv * (rw_even + skew) : 4 * (rw_even + skew) + (wv - 4) * (rw_even - skew);   // my first row in a sub-window
        const int buf = t & 1;
        const int64_t w = (int64_t)t - sn.t_init - 1;
        const int64_t sb0 = w * Kb + (int64_t)by * BR;                                 // global step of the block's first row
        auto dwin = glb(pa.dwin) + ((size_t)rep * 2 + buf) * Kb * qpad;
        auto scal = glb(pa.scal) + ((size_t)rep * 2 + buf) * Kb * 4;
        auto pval = glb(pa.pval) + ((size_t)rep * 2 + buf) * Kb * MCSAS_MAX_ACTIVE;
        auto povf = glb(pa.povf) + ((size_t)rep * 2 + buf) * Kb;
        auto gwin = glb(pa.gwin) + ((size_t)rep * 2 + buf) * Kb * W;
        double *gred = lds + pa.g.gram_off + 16;                                       // [2][8 waves][PIPE_GRAM_NT_MAX][256]
        constexpr size_t GRED = (size_t)PIPE_WAVES * PIPE_GRAM_NT_MAX * 256;
        const int nmine = nsb * RW;                                                    // my rows (<= 8), lane l <-> my l-th row
        const bool no_gram = MCSAS_TUNE_BITS(a) & 64;                                              // diagnostic: no Gram blocks (uniform)
        const int lrow = (lane / RW) * W + rbase + (lane % RW);                        // its offset in the block
        const bool lazy = pa.g.lazy_rows;
        PIPE_TLX_MARK(pa, t, 0);
        // ---- lazy rows: the block's stale `old` rows (their last proposal, N steps ago, was accepted: ~6 % of them) are
        // evaluated again from the parameter set, one q per thread and row — an eighth of a wave's row time for the whole
        // block, and no wave ends up with more rows than the others — and written back to the row cache.  Lanes 32 + l of
        // a wave mirror its lanes l: the same rows, their `old` side — validity flag and parameter set in one round trip
        // (under way while the proposals are drawn), and ONE prepare() call serves the proposals and the old sets.
        constexpr int CON = 12;                                   // doubles per Contrib record in LDS
        static_assert(sizeof(Contrib<M>) <= 8 * CON && sizeof(Contrib<M>) % 8 == 0, "Contrib record");
        int32_t *stl = reinterpret_cast<int32_t *>(gred);         // [0] count (zeroed before the tables' barrier), then the stale contributions
        double *scon = gred + 64;                                 // their Contrib records
        double prow[MCSAS_MAX_ACTIVE] = {0., 0., 0., 0.};
        const int l2 = lane - 32;
        const bool old_lane = lazy && l2 >= 0 && l2 < nmine;
        int stale_r = -1;
        if (old_lane) {
            const int lrow_o = (l2 / RW) * W + rbase + (l2 % RW);
            if (sb0 + lrow_o < max_iter) {
                const int r = (int)((sb0 + lrow_o) % N);
                const int v = row_valid[r];
#pragma unroll
                for (int p = 0; p < MCSAS_MAX_ACTIVE; ++p) if (p < P) prow[p] = rset[(size_t)r * P + p];
                if (!v) stale_r = r;
            }
        }
        int pov = 0, my_oslot = 0, my_sslot = 0;
        {
            const int r = (int)((sb0 + lrow) % N);
            if (lane < nmine) {
                if (lazy) my_oslot = r;
                else { my_oslot = slot_of[r]; my_sslot = stage[buf * Kb + by * BR + lrow]; }
            }
            const int64_t sl = sb0 + lrow;
#pragma unroll
            for (int p = 0; p < MCSAS_MAX_ACTIVE; ++p)
                if (p < P) {
                    double u = 0.5;
                    if (lane < nmine && sl < max_iter) u = src.at(sn.step_base + (uint64_t)sl * P + p, pov);
                    const double pv = gen_transform(a.gen_kind[p], u) * (a.gen_hi[p] - a.gen_lo[p]) + a.gen_lo[p];
                    if (!(old_lane && sb0 + ((l2 / RW) * W + rbase + (l2 % RW)) < max_iter)) prow[p] = pv;
                }
        }
        Contrib<M> prop;
        prop.prepare(a.model, prow);
        PIPE_TLX_MARK(pa, t, 1);
        int nst = 0;
        if (lazy) {
            if (stale_r >= 0) {
                const int e = atomicAdd(&stl[0], 1);
                stl[1 + e] = stale_r;
                double tmp[CON] = {};
                __builtin_memcpy(tmp, &prop, sizeof(Contrib<M>));
#pragma unroll
                for (int i = 0; i < (int)(sizeof(Contrib<M>) / 8); ++i) scon[e * CON + i] = tmp[i];
            }
            PIPE_LDS_BARRIER();
            nst = stl[0];
            for (int i = 0; i < nst; ++i) {                       // (list order varies from run to run, the rows do not depend on it)
                const int r = stl[1 + i];
                Contrib<M> c;
                {
                    double tmp[CON];
#pragma unroll
                    for (int x = 0; x < (int)(sizeof(Contrib<M>) / 8); ++x) tmp[x] = scon[i * CON + x];
                    __builtin_memcpy(&c, tmp, sizeof(Contrib<M>));
                }
#pragma unroll
                for (int x = 0; x < QTB; ++x) {
                    const int iq = tid + PIPE_BLOCK * x;
                    if (iq < qpad) cache[(size_t)r * qpad + iq] = pipe_point_intensity<M>(c, lq[iq], lq3[iq], tab);
                }
                if (tid == 0) row_valid[r] = 1;
            }
            if (nst) __syncthreads();                             // the refreshed rows have landed before the row loop loads them (uniform)
            else PIPE_LDS_BARRIER();                              // (the stale list shares the reduction buffer: read by all before it is reused)
        }
        PIPE_TLX_MARK(pa, t, 2);
        PIPE_TLX_MARK(pa, t, 3);
        // proposals and replay-overflow flags of all my rows: one store per wave (lane l <-> my l-th row)
        if (lane < nmine) {
            const int k = by * BR + lrow;
#pragma unroll
            for (int p = 0; p < MCSAS_MAX_ACTIVE; ++p) if (p < P) pval[k * MCSAS_MAX_ACTIVE + p] = prow[p];
            povf[k] = pov;
        }
        auto nvalid_of = [&](int ss) {
            const int64_t left = max_iter - (w * Kb + (int64_t)(by * nsb + ss) * W);
            return left >= W ? W : (left > 0 ? (int)left : 0);
        };
        if (pa.g.gram_lds) {
            // ---- default: sub-window by sub-window — every wave evaluates its rows of the sub-window (d also into the LDS row
            // buffer), barrier, the eight waves take the Gram block from LDS, next sub-window.  Only the LDS traffic is waited
            // for at the barriers: the rows' global stores drain behind the MFMAs.
            const int dstr = qpad + PIPE_DROW_PAD;
            double *dbuf = lds + pa.g.drow_off;
            double ocur[QPL], onext[QPL];
            {
                const auto orow0 = cache + (size_t)__builtin_amdgcn_readlane(my_oslot, 0) * qpad + lane;
#pragma unroll
                for (int j = 0; j < QPL; ++j) ocur[j] = orow0[WAVE * j];
            }
            PIPE_PIN_ROW(ocur);                                   // (a pending load carried into the loop would be waited for at its head, every iteration)
            for (int ss = 0; ss < nsb; ++ss) {
                for (int jr = 0; jr < RW; ++jr) {
                    const int l = ss * RW + jr, bl = __builtin_amdgcn_readfirstlane(l);
                    const int kl = ss * W + rbase + jr, k = by * BR + kl;
                    const Contrib<M> cnew = prop.bcast(bl);
                    const int sslot = __builtin_amdgcn_readlane(my_sslot, bl);
                    double d[QPL], nwv[QPL];
                    {
                        const int bn = __builtin_amdgcn_readfirstlane(l + 1 < nmine ? l + 1 : l);
                        const auto orow = cache + (size_t)__builtin_amdgcn_readlane(my_oslot, bn) * qpad + lane;
#pragma unroll
                        for (int j = 0; j < QPL; ++j) onext[j] = orow[WAVE * j];
                    }
                    // (a row behind max_iter — the last window of a run only — is evaluated like any other: its proposal is the
                    // generators' midpoint, its stores land in slots nobody reads, the Gram block masks it)
                    const auto nrow = cache + (size_t)sslot * qpad + lane;
                    const auto dr = dwin + (size_t)k * qpad + lane;
                    double *dl = dbuf + (size_t)(rbase + jr) * dstr + lane;
                    RowEval<M, QPL>::run(cnew, qt, lane, nwv);
#ifdef MCSAS_STAMPS                                               /* marks 4..11: my first four rows — evaluated / `old` rows there and stores out */
                    if (l < 4) { PIPE_PIN_ROW(nwv); PIPE_TL_MARK(pa, t, 4 + 2 * l); }
#endif
                    PIPE_PIN_ROW(ocur); PIPE_PIN_ROW(onext); PIPE_PIN_ROW(nwv);   // both `old` rows have landed before the first store is issued
                    double s1 = 0., s2 = 0.;
#pragma unroll
                    for (int j = 0; j < QPL; ++j) {
                        const int iq = lane + WAVE * j;
                        if (!lazy) nrow[WAVE * j] = nwv[j];
                        d[j] = nwv[j] - ocur[j];
                        dr[WAVE * j] = d[j];
                        dl[WAVE * j] = d[j];
                        s1 = fma(lw[iq], d[j], s1); s2 = fma(lwI[iq], d[j], s2);
                    }
                    // a = sum w d (even lanes), e = sum wI d (odd lanes); g = sum w d^2 is the Gram block's diagonal
                    const double ae = wave_sum2_split(s1, s2, lane);
                    if (lane < 2) scal[(size_t)k * 4 + lane] = ae;
#pragma unroll
                    for (int j = 0; j < QPL; ++j) ocur[j] = onext[j];
#ifdef MCSAS_STAMPS
                    if (l < 4) PIPE_TL_MARK(pa, t, 5 + 2 * l);
#endif
                }
                PIPE_TL_MARK(pa, t, 2 * (ss < 4 ? ss : 3));
                if (!no_gram) PIPE_LDS_BARRIER();                 // the sub-window's rows are in LDS
                const int nvalid = nvalid_of(ss);
                if (nvalid > 0 && !no_gram)                       // uniform in the block
                    pipe_prod_gram_lds<QPL>(dbuf, dstr, W, nvalid, lw, gred, gwin + (size_t)(by * nsb + ss) * W * W,
                                            scal + (size_t)(by * BR + ss * W) * 4);
                // (the next sub-window's rows overwrite dbuf only behind the reduction's first barrier, which every wave
                // passes after its last operand read; gred is written again behind the next rows -> Gram barrier)
                PIPE_TL_MARK(pa, t, 2 * (ss < 4 ? ss : 3) + 1);
            }
            PIPE_TL_MARK(pa, t, 17);
            return;
        }
#ifdef MCSAS_TUNING                                           // the overlapped variant (pipe_geometry: bit 18) is a measurement build's
#include "pipe_prod_overlap.inc"
#endif
        PIPE_TL_MARK(pa, t, 17);
        return;
    }

}

}  // namespace mcsas
