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
    if (tid == 0) {
        *reinterpret_cast<int32_t *>(lds + pa.g.gram_off + 16) = 0;   // lazy rows: the block's stale-row count
        *reinterpret_cast<int32_t *>(lds + pa.g.gram_off) = 0;        // the next row of the block to hand out (row claims below)
    }
    __syncthreads();
    PIPE_TL_CLOCK(c_bar);
    PIPE_TL_PUT(pa, t, 22, c_entry); PIPE_TL_PUT(pa, t, 23, c_snap); PIPE_TL_PUT(pa, t, 24, c_tab); PIPE_TL_PUT(pa, t, 25, c_bar);
    const QTables qt = make_qtables<M>(a.model, lq, lq3, tab);
    if constexpr (RQ) { pipe_prod_rowq<M, QPL>(pa, hot, lds, qt, rep, by, gy, t, sn, own); return; }
    auto rset = glb(a.rset) + (size_t)rep * N * P;
    auto cache = glb(a.cache) + (size_t)rep * a.cache_rows * qpad;
    const DrawSource src MCSAS_CHAIN_DRAWS(a, rep);
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
            MCSAS_INITIAL_ROW(row, n, n < N, false, true, sn.init_base, ovf)
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
        // ---- the block's rows: nsb sub-windows of W, d = new - old straight to the window buffer, and the Gram block of
        // every sub-window (pipe_gram.h).
        const int W = pa.g.w, nsb = pa.g.sub_per_block, BR = nsb * W;
        const int buf = t & 1;
        const int64_t w = (int64_t)t - sn.t_init - 1;
        const int64_t sb0 = w * Kb + (int64_t)by * BR;                                 // global step of the block's first row
        auto dwin = glb(pa.dwin) + ((size_t)rep * 2 + buf) * Kb * qpad;
        auto scal = glb(pa.scal) + ((size_t)rep * 2 + buf) * Kb * 4;
        auto pval = glb(pa.pval) + ((size_t)rep * 2 + buf) * Kb * MCSAS_MAX_ACTIVE;
        auto povf = glb(pa.povf) + ((size_t)rep * 2 + buf) * Kb;
        auto gwin = glb(pa.gwin) + ((size_t)rep * 2 + buf) * Kb * W;
        double *gred = lds + pa.g.gram_off + 16;                                       // [2][8 waves][PIPE_GRAM_NT_MAX][256]
        const bool no_gram = MCSAS_TUNE_BITS(a) & 64;                                              // diagnostic: no Gram blocks (uniform)
        const bool lazy = pa.g.lazy_rows;
        PIPE_TLX_MARK(pa, t, 0);
        // ---- lazy rows: the block's stale `old` rows (their last proposal, N steps ago, was accepted: ~6 % of them) are
        // evaluated again from the parameter set, one q per thread and row — an eighth of a wave's row time for the whole
        // block, and no wave ends up with more rows than the others — and written back to the row cache.  The threads that
        // prepare the proposals are mirrored by threads that take the same rows' `old` side — validity flag and parameter set
        // in one round trip (under way while the proposals are drawn) — and ONE prepare() call serves the proposals and the
        // old sets.  A thread that finds its row stale puts it on the block's list (stale_push); stale_refresh, called by
        // every thread, works the list off.
        constexpr int CON = PIPE_PROP_DOUBLES;                    // doubles per Contrib record in LDS
        static_assert(sizeof(Contrib<M>) <= 8 * (CON - 1) && sizeof(Contrib<M>) % 8 == 0, "Contrib record");
        int32_t *stl = reinterpret_cast<int32_t *>(gred);         // [0] count (zeroed before the tables' barrier), then the stale contributions
        double *scon = gred + 64;                                 // their Contrib records
        auto stale_push = [&](int r, const Contrib<M> &c) {
            const int e = atomicAdd(&stl[0], 1);
            stl[1 + e] = r;
            double tmp[CON] = {};
            __builtin_memcpy(tmp, &c, sizeof(Contrib<M>));
#pragma unroll
            for (int i = 0; i < (int)(sizeof(Contrib<M>) / 8); ++i) scon[e * CON + i] = tmp[i];
        };
        auto stale_refresh = [&]() {
            PIPE_LDS_BARRIER();
            const int nst = stl[0];
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
        };
        auto nvalid_of = [&](int ss) {
            const int64_t left = max_iter - (w * Kb + (int64_t)(by * nsb + ss) * W);
            return left >= W ? W : (left > 0 ? (int)left : 0);
        };
        if (pa.g.gram_lds) {
            // ---- default: sub-window by sub-window — the waves evaluate the sub-window's rows (d also into the LDS row
            // buffer), barrier, waves 0-3 take the Gram block from LDS while waves 4-7 start on the next sub-window's rows (below; all
            // eight take it where there is no next sub-window), next sub-window.  Only the LDS traffic is waited for at the barriers: the rows' global stores drain behind the MFMAs.
            // No wave has rows of its own: a wave CLAIMS the block's rows one by one from a counter in LDS (one returning add
            // by lane 0), always the next row before it evaluates the current one, so that the next `old` row is under way a
            // row ahead.  The SIMD arbitrates oldest-first, so of two waves that share one the younger (4-7) is the slower; with a
            // fixed deal one of the two finished a sub-window alone, latency-bound (2.1 us a row against 1.15 per row and SIMD for
            // two waves), whatever the deal — the first sub-window starts with every wave waiting for an `old` row, the later ones
            // do not.  A row's values, its sums and its place in the row buffer do not depend on the wave that evaluates it.
            // A claim behind the sub-window is kept across the Gram phase (its `old` row stays in flight), one behind the block
            // ends the wave's rows.
            const int dstr = qpad + PIPE_DROW_PAD;
            double *dbuf = lds + pa.g.drow_off;
            double *prec = lds + pa.g.rec_off;                    // [BR][CON] the block's proposals; a record's last double: `old` row slot, spare slot (eager rows)
            int32_t *claim = reinterpret_cast<int32_t *>(lds + pa.g.gram_off);   // (zeroed before the tables' barrier)
            auto take = [&]() {
                int v = 0;
                if (lane == 0) v = __hip_atomic_fetch_add(claim, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                return __builtin_amdgcn_readfirstlane(v);
            };
            int kc = take();                                      // my first row (the round trip runs beside the proposals)
            // the block's proposals, each worked out once: thread k < BR row k, thread 64 + k the `old` side of row k
            const int kk = tid & 63;
            const int64_t sl = sb0 + kk;
            const bool prop_thr = tid < BR, old_thr = lazy && tid >= 64 && tid - 64 < BR && sl < max_iter;
            const int rk = (int)(sl % N);
            double prow[MCSAS_MAX_ACTIVE] = {0., 0., 0., 0.};
            int stale_r = -1, pov = 0;
            if (old_thr) {
                const int v = row_valid[rk];
#pragma unroll
                for (int p = 0; p < MCSAS_MAX_ACTIVE; ++p) if (p < P) prow[p] = rset[(size_t)rk * P + p];
                if (!v) stale_r = rk;
            }
#pragma unroll
            for (int p = 0; p < MCSAS_MAX_ACTIVE; ++p)
                if (p < P) {
                    double u = 0.5;
                    if (prop_thr && sl < max_iter) u = src.at(sn.step_base + (uint64_t)sl * P + p, pov);
                    const double pv = draw_value(a, p, u);
                    if (!old_thr) prow[p] = pv;
                }
            Contrib<M> prop;
            prop.prepare(a.model, prow);
            PIPE_TLX_MARK(pa, t, 1);
            if (prop_thr) {
                double tmp[CON] = {};
                __builtin_memcpy(tmp, &prop, sizeof(Contrib<M>));
#pragma unroll
                for (int i = 0; i < (int)(sizeof(Contrib<M>) / 8); ++i) prec[kk * CON + i] = tmp[i];
                if (!lazy) {
                    int32_t *slots = reinterpret_cast<int32_t *>(prec + kk * CON + CON - 1);
                    slots[0] = slot_of[rk]; slots[1] = stage[buf * Kb + by * BR + kk];
                }
                // proposals and replay-overflow flags of the block's rows: one store (long done when the first `old` row is waited for)
                const int k = by * BR + kk;
#pragma unroll
                for (int p = 0; p < MCSAS_MAX_ACTIVE; ++p) if (p < P) pval[k * MCSAS_MAX_ACTIVE + p] = prow[p];
                povf[k] = pov;
            }
            if (stale_r >= 0) stale_push(stale_r, prop);
            if (lazy) stale_refresh();
            else PIPE_LDS_BARRIER();                              // the records are in LDS
            PIPE_TLX_MARK(pa, t, 2);
            PIPE_TLX_MARK(pa, t, 3);
            // the `old` row of row k of the block: lazy rows keep contribution r in slot r, r = (sb0 + k) % N (BR <= N / 2: one wrap)
            const int r0 = (int)(sb0 % N);
            auto oslot_of = [&](int k) {
                if (lazy) return r0 + k < N ? r0 + k : r0 + k - N;
                return __builtin_amdgcn_readfirstlane(reinterpret_cast<const int32_t *>(prec + k * CON + CON - 1)[0]);
            };
            double ocur[QPL], onext[QPL];
            {
                const auto orow0 = cache + (size_t)oslot_of(kc < BR ? kc : BR - 1) * qpad + lane;
#pragma unroll
                for (int j = 0; j < QPL; ++j) ocur[j] = orow0[WAVE * j];
            }
            PIPE_PIN_ROW(ocur);                                   // (a pending load carried into the loop would be waited for at its head, every iteration)
#ifdef MCSAS_STAMPS
            int nmine = 0;                                        // rows this wave has evaluated
#endif
            // Roles in the Gram phase (pipe_gram.h), chosen per sub-window (`split` below): waves 0-3 issue the MFMAs of sub-window ss,
            // waves 4-7 meanwhile go on with the row they hold a claim on — a row of sub-window ss + 1; one HELD row per wave —: d to
            // the window buffer and (a, e) to scal as ever, but d stays in registers while dbuf is still being read and goes to its LDS
            // row behind the barrier that ends the operand reads.  A wave whose claim lies behind sub-window ss + 1 goes straight to
            // that barrier.  The block's LAST sub-window (its only one where sub_per_block == 1) has no successor to hold a row of:
            // there the roles would only leave four waves idle and four with twice the operand work, so all eight are Gram waves, one
            // slice each.  Both forms fill the same eight partial slots, summed in the same order: the same bits.
            // Tuning bit 17: eight Gram waves and no held row in EVERY sub-window, as before the roles; bit 21: the roles in every
            // sub-window, the last one included (idle row waves there), as before they were chosen per sub-window.  Word 0, bit 17 and
            // bit 21 are three forms inside one measurement library: AB_WORDS=0,0x200000 tools/ab_pair.py <tuning> <tuning>.
            // s_barriers per sub-window, the same for EVERY wave of the block (ss, nsb, W, nvalid, no_gram and the tuning word are uniform
            // in the block, and so is `split`, which depends on nothing else — not on a wave's claim; a wave's role, its claim and
            // whether it holds a row change what it does BETWEEN barriers only):
            //   no_gram                      0
            //   nvalid == 0                  1   rows -> Gram (the Gram block is skipped by all waves: nobody holds a row either)
            //   else                         1 + (2 R - 1), R = ceil(tiles / PIPE_GRAM_TILES_PER_ROUND) rounds of the reduction
            //                                (pipe_prod_gram_lds_t: matrix waves, row waves with or without a held row, and the eight
            //                                Gram waves of an unsplit sub-window all pass the same 2 R - 1)
            // The row loop itself has no barrier: a wave that claims no row of a sub-window passes the same ones.
            const bool roles = !(MCSAS_TUNE_BITS(a) & (1 << 17)), roles_last = MCSAS_TUNE_BITS(a) & (1 << 21);
            const bool upper_wave = __builtin_amdgcn_readfirstlane(wave) >= WPB / 2;
            // one row of the block: the wave's claim kc, which belongs to sub-window sr; HOLD: no LDS copy, d is the caller's to keep
            auto eval_row = [&](int sr, auto hold, double (&d)[QPL]) {
                const int kn = take();
                const int k = by * BR + kc;
                Contrib<M> cnew;
                int sslot = 0;
                {
                    Contrib<M> cl;
                    double tmp[CON];
#pragma unroll
                    for (int i = 0; i < (int)(sizeof(Contrib<M>) / 8); ++i) tmp[i] = prec[kc * CON + i];   // one address for the wave
                    __builtin_memcpy(&cl, tmp, sizeof(Contrib<M>));
                    cnew = cl.bcast(0);
                    if (!lazy) sslot = __builtin_amdgcn_readfirstlane(reinterpret_cast<const int32_t *>(prec + kc * CON + CON - 1)[1]);
                }
                double nwv[QPL];
                {
                    const auto orow = cache + (size_t)oslot_of(kn < BR ? kn : kc) * qpad + lane;
#pragma unroll
                    for (int j = 0; j < QPL; ++j) onext[j] = orow[WAVE * j];
                }
                // (a row behind max_iter — the last window of a run only — is claimed and evaluated like any other: its proposal
                // is the generators' midpoint, its stores land in slots nobody reads, the Gram block masks it)
                const auto nrow = cache + (size_t)sslot * qpad + lane;
                const auto dr = dwin + (size_t)k * qpad + lane;
                double *dl = dbuf + (size_t)(kc - sr * W) * dstr + lane;
                RowEval<M, QPL>::run(cnew, qt, lane, nwv);
#ifdef MCSAS_STAMPS                                               /* marks 4..11: the first four rows I claimed — evaluated / `old` rows there and stores out */
                if (nmine < 4) { PIPE_PIN_ROW(nwv); PIPE_TL_MARK(pa, t, 4 + 2 * nmine); }
#endif
                PIPE_PIN_ROW(ocur); PIPE_PIN_ROW(onext); PIPE_PIN_ROW(nwv);   // both `old` rows have landed before the first store is issued
                double s1 = 0., s2 = 0.;
#pragma unroll
                for (int j = 0; j < QPL; ++j) {
                    const int iq = lane + WAVE * j;
                    if (!lazy) nrow[WAVE * j] = nwv[j];
                    d[j] = nwv[j] - ocur[j];
                    dr[WAVE * j] = d[j];
                    if constexpr (!decltype(hold)::value) dl[WAVE * j] = d[j];
                    s1 = fma(lw[iq], d[j], s1); s2 = fma(lwI[iq], d[j], s2);
                }
                // a = sum w d (even lanes), e = sum wI d (odd lanes); g = sum w d^2 is the Gram block's diagonal
                const double ae = wave_sum2_split(s1, s2, lane);
                if (lane < 2) scal[(size_t)k * 4 + lane] = ae;
#pragma unroll
                for (int j = 0; j < QPL; ++j) ocur[j] = onext[j];
#ifdef MCSAS_STAMPS
                if (nmine < 4) PIPE_TL_MARK(pa, t, 5 + 2 * nmine);
                ++nmine;
#endif
                kc = kn;
            };
            for (int ss = 0; ss < nsb; ++ss) {
                while (kc < (ss + 1) * W) {
                    double d[QPL];
                    eval_row(ss, std::false_type{}, d);
                }
                PIPE_TL_MARK(pa, t, 2 * (ss < 4 ? ss : 3));
                if (!no_gram) PIPE_LDS_BARRIER();                 // the sub-window's rows are in LDS
                const int nvalid = nvalid_of(ss);
                if (nvalid > 0 && !no_gram) {                     // uniform in the block
                    const bool split = roles && (roles_last || ss + 1 < nsb);   // uniform in the block: a row of sub-window ss + 1 can be held
                    double dheld[QPL];
                    int kheld = -1;                               // the row this wave evaluates beside the MFMAs (uniform in the wave)
                    // (the claims are handed out in order, eight at most beyond a sub-window: the second bound holds for every W
                    // pipe_geometry picks and keeps the LDS row inside dbuf for any other)
                    if (split && upper_wave && kc < BR && kc < (ss + 2) * W) { kheld = kc; eval_row(ss + 1, std::true_type{}, dheld); }
                    pipe_prod_gram_lds<QPL>(dbuf, dstr, W, nvalid, lw, gred, gwin + (size_t)(by * nsb + ss) * W * W,
                                            scal + (size_t)(by * BR + ss * W) * 4, split, [&]() {
                                                if (kheld >= 0) {
                                                    double *dl = dbuf + (size_t)(kheld - (ss + 1) * W) * dstr + lane;
#pragma unroll
                                                    for (int j = 0; j < QPL; ++j) dl[WAVE * j] = dheld[j];
                                                }
                                            });
                }
                // (the next sub-window's rows — a held one first — overwrite dbuf only behind the barrier of the reduction's last
                // round, which every wave passes after the last operand read; gred is written again behind the next rows -> Gram barrier)
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
