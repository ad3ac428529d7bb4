// pipe_scan.h — scan block of the pipeline (chain_pipe.h): the accept / reject decisions of a window, one workgroup per chain.
#pragma once
#include "pipe_prod.h"      // load_row_pairs, load_snap / store_snap, PIPE_LDS_BARRIER

namespace mcsas {

// Keep a wave-uniform double in a VGPR: the scan loop has far more uniform fp64 state than the 102
// SGPRs can hold, and spilled SGPRs come back one v_readlane at a time on the critical path.
#define MCSAS_IN_VGPR(x) asm volatile("" : "+v"(x))

// ------------------------------------------------------------------------------------ scanner
// LDS: two Gram blocks, ft and w*ft, the window's scalars, h of the current sub-window, flags and slot tables
template <int M, int QPL, int RPS, bool RQ>                    // RPS = rows per wave and sub-window (W / 8), compile time: see `request`
__device__ __forceinline__ void pipe_scan_block(const PipeArgs &pa, double *lds, int rep, int t, int stop_now) {
    static_assert(PIPE_GRAM_TILES_PER_ROUND * 256 == PIPE_BLOCK, "Gram reduction maps one thread to one tile element");
    const ChainArgs &a = pa.c;
    // the wave index is wave-uniform: keep it (and the row bookkeeping that hangs on it) on the scalar unit
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int N = a.n_contrib, P = a.model.n_active, qpad = a.qpad, Kb = pa.g.kb, W = pa.g.w;
    constexpr int T = PIPE_BLOCK;
    MCSAS_GLOBAL PipeChain &ch = glb(pa.chains)[rep];
    if (ch.done) return;                                      // uniform for the block
    if (RQ && tid == 0) pa.rowq[(size_t)rep * 2 + (t & 1)] = 0;   // the queue of PROD(t + 2) (this launch's producers use the other parity)
    MCSAS_STAMP_DECL(sb0 = 0, sb1 = 0, sb2 = 0, sb3 = 0);
    MCSAS_STAMP(sb0);
#ifdef MCSAS_STAMPS
    const uint64_t wc0 = wall_clock64();
#endif
    const PipeSnap sn = load_snap(&pa.chains[rep].snap[(t + 1) & 1]);   // the record in force for tick t (written at t-1; host for t = 0)

    double *rowbuf = lds;                                     // [W][qpad] d rows of the current sub-window (accepted ones are applied from here)
    double *Gl = rowbuf + (size_t)W * qpad;                   // [2][W*W] Gram block of the current / next sub-window
    double *lft = Gl + 2 * (size_t)W * W;                     // [qpad] ft, q-indexed
    double *lwft = lft + qpad;                                // [qpad] w * ft
    double *ssub = lwft + qpad;                               // [Kb][4] a, e, g of every step of the window
    double *hsub = ssub + (size_t)Kb * 4;                     // [64] h of the current sub-window, by step offset
    int32_t *osub = reinterpret_cast<int32_t *>(hsub + 64);   // [Kb] replay-overflow flags
    int32_t *lstage = osub + Kb, *lslot = lstage + Kb;        // [Kb] spare row slot of step k / row slot of its contribution
    int32_t *lacc = lslot + Kb;                               // [Kb + 1] accepted steps of this window, count in lacc[Kb]
    int32_t *sacc = lacc + Kb + 1;                            // [1 + 64] this sub-window: count, then the accepted steps' offsets in it
    int32_t *ctl = sacc + 1 + 64;                             // [4]: [2] = live
    double *lwq = reinterpret_cast<double *>((reinterpret_cast<unsigned long long>(ctl + 4) + 7ull) & ~7ull);   // [qpad] w (row queues: the Gram blocks are taken here)
    auto gft = glb(pa.ft) + (size_t)rep * qpad, gwft = glb(pa.wft) + (size_t)rep * qpad;
    auto rset = glb(a.rset) + (size_t)rep * N * P;
    auto cache = glb(a.cache) + (size_t)rep * a.cache_rows * qpad;
    const int buf = t & 1;
    const auto dwin = glb((const double *)pa.dwin) + ((size_t)rep * 2 + buf) * Kb * qpad;
    const auto gwin = glb((const double *)pa.gwin) + ((size_t)rep * 2 + buf) * Kb * W;
    const auto scal = glb((const double *)pa.scal) + ((size_t)rep * 2 + buf) * Kb * 4;
    const auto pval = glb((const double *)pa.pval) + ((size_t)rep * 2 + buf) * Kb * MCSAS_MAX_ACTIVE;
    const auto povf = glb((const int32_t *)pa.povf) + ((size_t)rep * 2 + buf) * Kb;
    auto slot_of = glb(pa.slot_of) + (size_t)rep * N;
    auto stage = glb(pa.stage_slot) + ((size_t)rep * 2 + buf) * Kb;
    const auto gw_ = glb(a.w), gwI_ = glb(a.wI), gI_ = glb(a.I);
    const double nqd = (double)a.nq;

    // scanner-side chain state (meaningful in wave 0)
    FitResult cur{ch.A, ch.b, ch.chi2};
    double SC = ch.SC, SIC = ch.SIC, SCC = ch.SCC;
    int64_t num_iter = ch.num_iter, num_moves = ch.num_moves;
    int stopped = ch.stopped, overflow = 0;
    bool attempt_over = false;
    double Xwin = 0.;                                           // chi²·Q at the end of this tick's window (PipeGeom::resum_every)
    bool had_window = false;

    if (t < sn.t_init) {
        // nothing scheduled for this chain at this tick; just republish below
    } else if (t == sn.t_init) {
        // ---- model.calc over the initial set: rows summed in contribution order (scatteringmodel.py:90-101)
        // One q per thread, the N rows in batches of 16 loads (one wave walking the rows one dependent load at a time took
        // ~100 us at N = 400: a fortieth of a 20 000-step launch); every q is summed in contribution order, as before.
        for (int i = tid; i < qpad; i += T) {
            double f = 0.;
            int n = 0;
            for (; n + 16 <= N; n += 16) {
                double v[16];
#pragma unroll
                for (int k = 0; k < 16; ++k) v[k] = cache[(size_t)(n + k) * qpad + i];
#pragma unroll
                for (int k = 0; k < 16; ++k) f += v[k];
            }
            for (; n < N; ++n) f += cache[(size_t)n * qpad + i];
            lft[i] = f;
        }
        PIPE_LDS_BARRIER();                                    // (t == t_init for every thread of the block)
        if (wave == 0) {
            double ft[QPL];
#pragma unroll
            for (int j = 0; j < QPL; ++j) ft[j] = lft[lane + WAVE * j];
            double s1 = 0., s2 = 0., s3 = 0.;
#pragma unroll
            for (int j = 0; j < QPL; ++j) {
                const double wf = gw_[lane + WAVE * j] * ft[j];
                s1 += wf; s2 = fma(wf, ft[j], s2); s3 = fma(gwI_[lane + WAVE * j], ft[j], s3);
                gft[lane + WAVE * j] = ft[j]; gwft[lane + WAVE * j] = wf;
                lft[lane + WAVE * j] = ft[j];                 // the end-of-attempt code below reads ft from LDS
            }
            wave_sum3(s1, s2, s3);
            SC = s1; SCC = s2; SIC = s3;
            cur = solve_fit(a, SC, SCC, SIC);
            num_iter = 0; num_moves = 0;
            if (N <= 1 || a.max_iter <= 0 || !(cur.chi2 > a.conv_crit)) attempt_over = true;
        }
    } else {
        // ---- window w = t - t_init - 1, sub-window by sub-window
        const int64_t w = (int64_t)t - sn.t_init - 1;
        const int64_t budget = a.max_iter - w * Kb;
        const int kmax_all = budget < Kb ? (budget < 0 ? 0 : (int)budget) : Kb;
        const int ri0 = (int)((w * Kb) % N);
        const int nsub = (kmax_all + W - 1) / W;
        // The d rows travel HBM/L2 -> registers -> (dot product with w ft) -> LDS row buffer.  A wave owns the rows
        // wave, wave + 8, ... of a sub-window (RPS of them).
        // Row i of EVERY sub-window sits in register set i, and the row for the next sub-window is requested as soon as
        // the set has been used: RPS rows per wave are under way all the time, also across the decision and apply
        // phases.  RPS is a template parameter because a load whose target depends on a run-time choice (or sits
        // under a condition) becomes a load into scratch registers, a wait and a copy at the join: no prefetch.
        const int total_r = nsub * RPS;
        int r_load = 0;
        double rs[RPS][QPL];
        auto request = [&](double (&dst)[QPL]) {
            const int rr = r_load < total_r ? r_load : 0;      // (past the end: row 0 again, never used)
            const int k = (rr / RPS) * W + wave + 8 * (rr % RPS);
            load_row_pairs<QPL>(dwin + (size_t)(k < kmax_all ? k : 0) * qpad, lane, dst);
            ++r_load;
        };
#pragma unroll
        for (int i = 0; i < RPS; ++i) request(rs[i]);
        // Gram block of sub-window s -> LDS buffer s & 1 (W*W doubles, contiguous in HBM): the loads are issued at the
        // top of the previous sub-window and parked in registers, the LDS stores follow behind that sub-window's rows
        // (a load-store copy loop would drain every outstanding row load at its first store)
        constexpr int NG = (RPS * RPS * 64 / 2 + T - 1) / T;   // 16-byte pieces per thread (W*W / 2 pieces in all)
        v2f64 gtmp[NG];
        auto gram_fetch = [&](int s) {
            const auto src = gwin + (size_t)s * W * W;
#pragma unroll
            for (int x = 0; x < NG; ++x) {
                int i = 2 * (tid + T * x);
                if (i > W * W - 2) i = W * W - 2;              // (clamped, not skipped: see `request`)
                gtmp[x] = *(const MCSAS_GLOBAL v2f64 *)(src + i);
            }
        };
        auto gram_store = [&](int s) {
            double *dst = Gl + (size_t)(s & 1) * W * W;
#pragma unroll
            for (int x = 0; x < NG; ++x) {
                const int i = 2 * (tid + T * x);
                if (i < W * W) *reinterpret_cast<v2f64 *>(dst + i) = gtmp[x];
            }
        };
        constexpr bool gram_here = RQ;                         // rows with an integral: the Gram blocks are worked out below, from the rows in LDS
        if (nsub > 0 && !gram_here) { gram_fetch(0); gram_store(0); }
        // ft, w ft -> LDS; the thread's own q in the apply phase: q = tid (+ 512)
        constexpr int QT = (QPL * 64 + T - 1) / T;            // q per thread in the apply phase (1 or 2)
        double wq[QT];
#pragma unroll
        for (int x = 0; x < QT; ++x) {
            const int i = tid + T * x;
            wq[x] = 0.;
            if (i < qpad) { wq[x] = gw_[i]; lft[i] = gft[i]; lwft[i] = gwft[i]; if constexpr (RQ) lwq[i] = wq[x]; }
        }
        static_assert(PIPE_BLOCK >= 512, "one window step per thread: pipe_geometry caps Kb at PIPE_BLOCK");
        if (tid < kmax_all) {                                  // Kb <= PIPE_BLOCK = threads (pipe_geometry)
            osub[tid] = povf[tid];
            if (!pa.g.lazy_rows) {                             // (lazy rows never move: no slot tables)
                int r = ri0 + tid; if (r >= N) r -= N;
                lstage[tid] = stage[tid]; lslot[tid] = slot_of[r];
            }
        }
        for (int i = tid; i < kmax_all * 4; i += T) ssub[i] = scal[i];
        if (tid == 0) { lacc[Kb] = 0; sacc[0] = 0; }
        const double invSw = 1.0 / a.Sw, SIoSw = a.SI / a.Sw, Scen = a.SII - a.SI * a.SI / a.Sw;
        const int resum = pa.g.resum_every;
        const bool swap_slots = !pa.g.lazy_rows;
        double X = resum ? ch.X : cur.chi2 * nqd;
        bool touched = false, live = true;
        int num_acc_win = 0;
        if (wave == 0) {
            if (stop_now) stopped = 1;                         // McSAS.stop as the host saw it when it launched this tick
            if (lane == 0) ctl[2] = (!(cur.chi2 > a.conv_crit) || stopped) ? 0 : 1;   // `live`, shared by all waves
        }
        PIPE_LDS_BARRIER();
        live = ctl[2] != 0;
        double wftp[QPL];
        load_row_pairs_lds<QPL>(lwft, lane, wftp);
        // loop-invariant fit constants and the running sums, pinned in VGPRs (see MCSAS_IN_VGPR)
        double cSII = a.SII, cSI = a.SI, cScen = Scen, cSIoSw = SIoSw, cinvSw = invSw, cCrit = a.conv_crit, cnq = nqd;
        MCSAS_IN_VGPR(cSII); MCSAS_IN_VGPR(cSI); MCSAS_IN_VGPR(cScen); MCSAS_IN_VGPR(cSIoSw); MCSAS_IN_VGPR(cinvSw);
        MCSAS_IN_VGPR(cCrit); MCSAS_IN_VGPR(cnq);
        MCSAS_IN_VGPR(SC); MCSAS_IN_VGPR(SIC); MCSAS_IN_VGPR(SCC); MCSAS_IN_VGPR(X);
        const bool find_bg = a.find_bg, pos_bg = a.pos_bg, never_accept = MCSAS_TUNE_BITS(a) & 32;
#ifdef MCSAS_STAMPS
        int64_t ph[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#endif
        MCSAS_STAMP_DECL(s0 = 0, s1 = 0, s2 = 0, s3 = 0, s4 = 0, s5 = 0);
        MCSAS_STAMP(sb1);
        for (int s = 0; s < nsub && live; ++s) {
            MCSAS_STAMP(s0);
            const int k0 = s * W;
            const int cnt = (kmax_all - k0) < W ? (kmax_all - k0) : W;
            if (!gram_here) gram_fetch(s + 1 < nsub ? s + 1 : s);   // (its LDS buffer was last read two sub-windows ago)
            // ---- my rows of this sub-window: h = Σ (w ft) d, and the row itself into the LDS row buffer
            double acc[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) acc[i] = 0.;
            auto use_row = [&](int i, const double (&row)[QPL]) {
                double h0 = 0., h1 = 0.;
#pragma unroll
                for (int j = 0; j < QPL; j += 2) {
                    h0 = fma(wftp[j], row[j], h0);
                    if (j + 1 < QPL) h1 = fma(wftp[j + 1], row[j + 1], h1);
                }
                const double hs = h0 + h1;
#pragma unroll
                for (int x = 0; x < 8; ++x) acc[x] = (x == i) ? hs : acc[x];
                const int g = wave + 8 * i;
                if (g < cnt) {
                    double *dst = rowbuf + (size_t)g * qpad;
                    if constexpr (QPL >= 2) {
#pragma unroll
                        for (int c = 0; c < QPL / 2; ++c)
                            *reinterpret_cast<v2f64 *>(dst + 128 * c + 2 * lane) = (v2f64){row[2 * c], row[2 * c + 1]};
                    } else {
                        dst[lane] = row[0];
                    }
                }
            };
#pragma unroll
            for (int i = 0; i < RPS; ++i) { use_row(i, rs[i]); request(rs[i]); }
            {
                // eight sums for the price of ~1.5: lane l < 8 ends up with the total of acc[4 (l&1) + 2 ((l>>1)&1) + ((l>>2)&1)]
                const double tot = wave_sum8_transposed(acc, lane);
                const int c = 4 * (lane & 1) + 2 * ((lane >> 1) & 1) + ((lane >> 2) & 1);
                if (lane < 8 && c < RPS && wave + 8 * c < cnt) hsub[wave + 8 * c] = tot;
            }
            if (!gram_here) gram_store(s + 1);                 // read at the earliest after B1 of the next sub-window
            MCSAS_STAMP(s1);
            PIPE_LDS_BARRIER();                                            // B1: hsub, the row buffer and this sub-window's Gram block complete
            if constexpr (gram_here) {
                // G[a][k] = Σ_q w d_a d_k of the sub-window's (eight) rows, which are all in the row buffer now: wave a takes row a
                // against every row, q = lane + 64 j, the eight sums reduced together.  (The producers' MFMA pass did this when one
                // workgroup evaluated the eight steps of a sub-window; with rows pulled from a queue no workgroup has them all.)
                if (wave < cnt) {
                    double ga[8];
#pragma unroll
                    for (int x = 0; x < 8; ++x) ga[x] = 0.;
                    // (not unrolled over q: sixteen slots of nine operands each in flight took the scan loop's registers — 929 spills at
                    // Q = 1024 and a sub-window in 40 us instead of 5.  Rows behind cnt are stale LDS: their sums are never read.)
#pragma nounroll
                    for (int j = 0; j < QPL; ++j) {
                        const int iq = lane + WAVE * j;
                        const double wa = lwq[iq] * rowbuf[(size_t)wave * qpad + iq];
#pragma unroll
                        for (int x = 0; x < 8; ++x) ga[x] = fma(wa, rowbuf[(size_t)x * qpad + iq], ga[x]);
                    }
                    const double tot = wave_sum8_transposed(ga, lane);
                    const int c = 4 * (lane & 1) + 2 * ((lane >> 1) & 1) + ((lane >> 2) & 1);
                    if (lane < 8) Gl[(size_t)(s & 1) * W * W + (size_t)wave * W + c] = tot;
                }
                PIPE_LDS_BARRIER();
            }
            MCSAS_STAMP(s2);
            if (wave == 0) {
                // ---- the W decisions of the sub-window: lane g <-> step k0 + g
                __builtin_amdgcn_s_setprio(1);
                const int g = lane;
                const bool in = g < cnt;
                const int kg = in ? k0 + g : k0;
                double h = hsub[in ? g : 0];
                const double sc0 = ssub[kg * 4 + 0], sc1 = ssub[kg * 4 + 1], sc2 = ssub[kg * 4 + 2];
                const int ovg = osub[kg];
                const double *Gs = Gl + (size_t)(s & 1) * W * W;
                int nacc_sub = 0;
                // One round per accepted step: every remaining candidate (lanes in `cmask`) is judged against the current
                // state at once, the first that passes is taken, the state moves on, again from the step behind it.  A round is
                // a dependent chain on ONE wave — early in a chain, when most proposals pass, the rounds are the whole tick —
                // so everything that is not on that chain is kept out of it: the candidate and overflow masks are scalars, the
                // fit flags are compile-time (three copies of the loop), the accepted steps are recorded as a bit mask and
                // published to LDS once per sub-window, chi²·Q of every candidate is divided out beside its comparison.
                auto decide = [&](auto fb_t, auto pb_t) {
                    constexpr bool FB = decltype(fb_t)::value, PB = decltype(pb_t)::value;
                    const unsigned long long inmask = cnt >= 64 ? ~0ull : ((1ull << cnt) - 1ull);
                    const unsigned long long ovm_all = __ballot(in && ovg) & inmask;
                    unsigned long long cmask = inmask, accm = 0ull, leftover = 0ull;
                    // The current state's chi²·Q enters a comparison as the pair (Na, Da), X = Sa - Na / Da, with (S - X, 1) at the
                    // head of a sub-window — "chi²_t < chi²" (mcsas.py:379), num² / den > Na / Da + (S - Sa), is taken across:
                    // num² Da > (Na + (S - Sa) Da) den.  With (S - X, 1) that is the very expression num² > (S - X) den; behind an
                    // accepted step it is that step's own (num², den), exact, and the division that gives X leaves the chain of
                    // dependent operations a round consists of (it is made once, when the sub-window is through).  S is the same
                    // for every candidate unless positiveBackground can switch a candidate to the uncentred sums.
                    double Sa = PB ? X : 0., Na = PB ? 0. : (FB ? cScen : cSII) - X, Da = 1.0;
                    MCSAS_IN_VGPR(Na); MCSAS_IN_VGPR(Da);
                    // Round 5: ONE exit (no candidate passes) and nothing in a round but the dependent chain itself — the step and
                    // overflow counts are taken from the masks behind the loop, the accepted candidate's own convergence test is made
                    // on its two numbers; a chain that ends inside the sub-window empties the candidate mask instead of leaving the
                    // loop (one more, empty, round at the very end of an attempt).  The loop went from ~125 to ~60 instructions a round.
                    for (;;) {
                        const double SCt = SC + sc0, SICt = SIC + sc1, SCCt = SCC + fma(2., h, sc2);
                        double S = cSII, num = SICt, den = SCCt;
                        if constexpr (FB) {
                            const double numc = fma(-cSIoSw, SCt, SICt), denc = fma(-(SCt * cinvSw), SCt, SCCt);
                            if constexpr (PB) {
                                const bool neg_b = fma(cSI, denc, -(numc * SCt)) < 0.;
                                if (!neg_b) { S = cScen; num = numc; den = denc; }
                            } else {
                                S = cScen; num = numc; den = denc;
                            }
                        }
                        const double n2 = num * num;
                        bool pass;
                        if constexpr (PB) {
                            pass = n2 * Da > fma(S - Sa, Da, Na) * den;
                        } else {
                            pass = n2 * Da > Na * den;
                        }
                        unsigned long long amask = __ballot(pass) & cmask;
                        if (never_accept) amask = 0ull;            // diagnostic: never accept
                        if (amask == 0ull) break;
                        const int ga = __builtin_ctzll(amask);
                        const unsigned long long upto = (2ull << ga) - 1ull;          // steps 0 .. ga
                        // the steps behind the accepted one see ft + d_acc: h_k += Σ w d_acc d_k (read issued first)
                        const double gk = Gs[(size_t)ga * W + (in ? g : 0)];
                        SC = readlane_f64(SCt, ga); SIC = readlane_f64(SICt, ga); SCC = readlane_f64(SCCt, ga);
                        Na = readlane_f64(n2, ga); Da = readlane_f64(den, ga);
                        double Sg = FB ? cScen : cSII;
                        if constexpr (PB) { Sa = readlane_f64(S, ga); MCSAS_IN_VGPR(Sa); Sg = Sa; }
                        h += gk;
                        accm |= 1ull << ga;
                        cmask &= ~upto;
                        // this candidate, accepted, ends the attempt: !(chi² > criterion), on its own (num², den)
                        // (the ballot tells the compiler that the test — the same in every lane — is wave-uniform: masks stay scalar)
                        if (__ballot(!((Sg - cCrit * cnq) * Da > Na)) != 0ull) { live = false; leftover = cmask; cmask = 0ull; }
                    }
                    {
                        const unsigned long long consumed = inmask & ~leftover;       // the steps this sub-window went through
                        num_iter += __builtin_popcountll(consumed);
                        num_moves += __builtin_popcountll(accm);
                        if (ovm_all & consumed) overflow = 1;
                    }
                    // the accepted steps of the sub-window, in order: sacc[1 + i] = step in the sub-window, lacc[...] = step in the window
                    nacc_sub = __builtin_popcountll(accm);
                    if (nacc_sub) {
                        X = (PB ? Sa : (FB ? cScen : cSII)) - Na / Da;   // chi²·Q of the state the sub-window ends in
                        MCSAS_IN_VGPR(X);
                        touched = true;
                    }
                    if ((accm >> lane) & 1ull) {
                        const int pos = __builtin_popcountll(accm & ((1ull << lane) - 1ull));
                        const int acc_row = k0 + lane;
                        sacc[1 + pos] = lane;
                        lacc[num_acc_win + pos] = acc_row;
                        if (swap_slots) {                          // slot swap: rows are never copied (lazy rows never move: nothing to swap)
                            const int fresh = lstage[acc_row], freed = lslot[acc_row];
                            lslot[acc_row] = fresh; lstage[acc_row] = freed;
                        }
                    }
                    num_acc_win += nacc_sub;
                };
                if (!find_bg) decide(std::false_type{}, std::false_type{});
                else if (pos_bg) decide(std::true_type{}, std::true_type{});
                else decide(std::true_type{}, std::false_type{});
                cur.chi2 = X / cnq;                               // scale and background are only needed at the end of the attempt
                if (lane == 0) { sacc[0] = nacc_sub; ctl[2] = live ? 1 : 0; }
                __builtin_amdgcn_s_setprio(0);
            }
            MCSAS_STAMP(s3);
            PIPE_LDS_BARRIER();                                            // B2: decisions published
            MCSAS_STAMP(s4);
            live = ctl[2] != 0;
            const int nacc = sacc[0];
            if (nacc > 0) {
                // ---- ft += d for the accepted steps, in order (mcsas.py:381), straight from the LDS row buffer: no
                // memory round trip on the way to the next sub-window.  (d = new - old is the producers' fp64
                // difference; the wavefront kernel's (ft - old) + new differs from ft + d in the last bit at most.)
#pragma unroll
                for (int x = 0; x < QT; ++x) {
                    const int i = tid + T * x;
                    if (i < qpad) {
                        double f = lft[i];
                        int n = 0;
                        // (four rows at a time: their LDS reads are independent, the additions keep their order — early in a chain a
                        // sub-window has a dozen accepted rows and a dependent read per row was a third of the tick's apply phase)
                        for (; n + 4 <= nacc; n += 4) {
                            const int r0 = sacc[1 + n], r1 = sacc[2 + n], r2 = sacc[3 + n], r3 = sacc[4 + n];
                            const double v0 = rowbuf[(size_t)r0 * qpad + i], v1 = rowbuf[(size_t)r1 * qpad + i];
                            const double v2 = rowbuf[(size_t)r2 * qpad + i], v3 = rowbuf[(size_t)r3 * qpad + i];
                            f += v0; f += v1; f += v2; f += v3;
                        }
                        for (; n < nacc; ++n) f += rowbuf[(size_t)sacc[1 + n] * qpad + i];
                        lft[i] = f; lwft[i] = wq[x] * f;
                    }
                }
                PIPE_LDS_BARRIER();                                        // B3: ft complete; sacc and the row buffer may be rewritten
                load_row_pairs_lds<QPL>(lwft, lane, wftp);
            }
            if (resum && wave == 0 && live && num_iter % resum == 0) {
                // (rows with an integral) every `resum` steps of the attempt — wherever that falls in a window — the running
                // sums are re-derived from ft so that the incremental updates cannot drift; ft is complete here (B3, or
                // nothing was accepted in this sub-window)
                double s1 = 0., s2 = 0., s3 = 0.;
#pragma unroll
                for (int j = 0; j < QPL; ++j) {
                    const double f = lft[lane + WAVE * j], wf = lwft[lane + WAVE * j];
                    s1 += wf; s2 = fma(wf, f, s2); s3 = fma(gwI_[lane + WAVE * j], f, s3);
                }
                wave_sum3(s1, s2, s3);
                SC = s1; SCC = s2; SIC = s3;
                cur = solve_fit(a, SC, SCC, SIC);
                X = cur.chi2 * nqd;
            }
#ifdef MCSAS_STAMPS
            MCSAS_STAMP(s5);
            ph[0] += s1 - s0; ph[1] += s2 - s1; ph[2] += s3 - s2; ph[3] += s4 - s3; ph[4] += s5 - s4; ph[5] += 1; ph[6] += nacc;
#endif
        }
        MCSAS_STAMP(sb2);
#ifdef MCSAS_STAMPS
        if (wave == 0 && lane == 0) for (int i = 0; i < 8; ++i) ch.dbg[i] += ph[i];
#endif
        if (wave == 0 && lane == 0) lacc[Kb] = num_acc_win;
        PIPE_LDS_BARRIER();
        {   // write the window's slot tables back and store the accepted proposals (mcsas.py:381), all waves
            const int nacc = lacc[Kb];
            if (nacc > 0) {
                if (!pa.g.lazy_rows) {
                    for (int i = tid; i < kmax_all; i += T) {
                        stage[i] = lstage[i];
                        int r = ri0 + i; if (r >= N) r -= N;
                        slot_of[r] = lslot[i];
                    }
                } else {
                    // the accepted contributions' cached rows are stale from here on (the producer that proposes for them
                    // next, N steps from now, evaluates them again from the parameters stored just below)
                    auto row_valid = glb(pa.row_valid) + (size_t)rep * N;
                    for (int i = tid; i < nacc; i += T) {
                        int r = ri0 + lacc[i]; if (r >= N) r -= N;
                        row_valid[r] = 0;
                    }
                }
                for (int i = tid; i < nacc * P; i += T) {
                    const int kk = lacc[i / P], p = i % P;
                    int r = ri0 + kk; if (r >= N) r -= N;
                    rset[(size_t)r * P + p] = pval[(size_t)kk * MCSAS_MAX_ACTIVE + p];
                }
                // park ft in HBM for the next tick
                for (int i = tid; i < qpad; i += T) { gft[i] = lft[i]; gwft[i] = lwft[i]; }
            }
        }
        if (wave == 0) {
            Xwin = X; had_window = true;
            if (touched && !resum) {
                // re-sum the fit sums from ft so the incremental updates cannot drift
                double s1 = 0., s2 = 0., s3 = 0.;
#pragma unroll
                for (int j = 0; j < QPL; ++j) {
                    const double f = lft[lane + WAVE * j], wf = lwft[lane + WAVE * j];
                    s1 += wf; s2 = fma(wf, f, s2); s3 = fma(gwI_[lane + WAVE * j], f, s3);
                }
                wave_sum3(s1, s2, s3);
                SC = s1; SCC = s2; SIC = s3;
                cur = solve_fit(a, SC, SCC, SIC);
            }
            if (!(cur.chi2 > a.conv_crit) || !(num_iter < a.max_iter) || stopped) attempt_over = true;
        }
    }

    // ---- bookkeeping by the scanner wave: end of attempt (mcsas.py:424-439), schedule record for t+2
    if (wave == 0) {
        PipeSnap next = sn;
        int done = 0;
        uint64_t draw_pos = ch.draw_pos;
        int64_t total_steps = ch.total_steps;
        int attempts = ch.attempts, converged = ch.converged;
        if (attempt_over) {
            double ft[QPL];
            double s1 = 0., s2 = 0., s3 = 0.;
#pragma unroll
            for (int j = 0; j < QPL; ++j) {
                ft[j] = lft[lane + WAVE * j];
                const double wf = gw_[lane + WAVE * j] * ft[j];
                s1 += wf; s2 = fma(wf, ft[j], s2); s3 = fma(gwI_[lane + WAVE * j], ft[j], s3);
            }
            wave_sum3(s1, s2, s3);
            cur = solve_fit(a, s1, s2, s3);
            double rs = 0.;
#pragma unroll
            for (int j = 0; j < QPL; ++j) {
                const int i = lane + WAVE * j;
                const double r = gI_[i] - (ft[j] * cur.A + cur.b);
                rs += gw_[i] * r * r;
            }
            cur.chi2 = wave_sum(rs) / nqd;                    // chiSqr, backgroundscalingfit.py:72-77
            converged = !(cur.chi2 > a.conv_crit);
            total_steps += num_iter;
            draw_pos = sn.step_base + (uint64_t)num_iter * P;
            if (converged || stopped || sn.attempt >= a.max_retries) {
                done = 1;
#pragma unroll
                for (int j = 0; j < QPL; ++j)
                    glb(a.fit)[(size_t)rep * qpad + lane + WAVE * j] = ft[j] * cur.A + cur.b;
                next.alive = 0;
            } else {
                ++attempts;
                next.attempt = sn.attempt + 1;
                next.t_init = t + 2;
                next.init_base = draw_pos;
                next.step_base = draw_pos + MCSAS_INITIAL_DRAWS(a, N, P);
                next.alive = 1;
            }
        }
        overflow = __any(overflow);
        MCSAS_STAMP(sb3);
#ifdef MCSAS_STAMPS
        if (lane == 0 && sb1 != 0) { ch.dbg[12] += sb1 - sb0; ch.dbg[13] += sb3 - sb2; ch.dbg[14] += 1; ch.dbg[15] += sb3 - sb0; }
        if (lane == 0) {
            if (ch.last_end) { ch.dbg[16] += (int64_t)(wc0 - ch.last_end); ch.dbg[17] += 1; }
            ch.dbg[18] += (int64_t)(wall_clock64() - wc0);
            ch.last_end = wall_clock64();
        }
#endif
        if (lane == 0) {
            store_snap(&pa.chains[rep].snap[t & 1], next);    // read by PROD(t+2) and SCAN(t+1)
            // a finished chain: the OTHER record's `alive` goes to 0 as well, so that the producers of the odd ticks stop
            // evaluating rows for it too (one word; a producer of this very launch that still reads 1 only does work nobody uses)
            if (done) glb(&pa.chains[rep].snap[(t + 1) & 1].alive)[0] = 0;
            ch.SC = SC; ch.SIC = SIC; ch.SCC = SCC; ch.A = cur.A; ch.b = cur.b; ch.chi2 = cur.chi2;
            ch.X = had_window ? Xwin : cur.chi2 * nqd;            // (no window this tick: the attempt's initial fit)
            ch.num_iter = num_iter; ch.num_moves = num_moves; ch.total_steps = total_steps;
            ch.draw_pos = draw_pos; ch.attempts = attempts; ch.converged = converged; ch.stopped = stopped;
            if (overflow) atomicOr(&pa.chains[rep].overflow, 1);
            if (done) {
                ch.done = 1;
                ChainOut o;
                o.chisq = cur.chi2; o.scaling = cur.A; o.background = cur.b;
                o.seconds = (double)(wall_clock64() - ch.t_start) * 1e-8;
                o.num_iter = num_iter; o.num_moves = num_moves; o.draws = (int64_t)draw_pos;
                o.total_steps = total_steps;
                o.attempts = attempts; o.converged = converged; o.stream_overflow = ch.overflow | overflow; o.stopped = stopped;
#ifdef MCSAS_STAMPS
                for (int i = 0; i < 20; ++i) o.dbg[i] = ch.dbg[i];
#endif
                a.out[rep] = o;
                if (__hip_atomic_fetch_add(pa.n_done_dev, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1 == a.n_reps)
                    __hip_atomic_store(pa.n_done, a.n_reps, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            }
        }
    }
}

}  // namespace mcsas
