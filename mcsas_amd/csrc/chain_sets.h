// chain_sets.h — one wavefront = one Monte-Carlo chain judged by SEVERAL data sets at once (mcsas_hip_analyse_sets,
// mcsas_hip_analyse_sets_mode): one population of contributions, one running intensity over the q-points of all sets, and at every fit
// (initial, per step, final) a least-squares scale and background of its own for each set.  The chain minimises the reduced chi² over
// all points,
//   chi²·Q = X = sum over the sets of (S_s - num_s²/den_s)      (the closed-form optimum of each set from its own five sums),
// and accepts a step iff X_t < X (strict, mcsas.py:379).  What it extends: McSAS.mcFit (mcsas.py:354-404) and
// BackgroundScalingFit.calc (backgroundscalingfit.py:112-139), which know one curve.
// SHARED (MCSAS_SETS_SCALE_SHARED): ONE scale for all sets, a background per set — the same per-set sums and pieces, meeting as
//   X = sum S_s - (sum num_s)² / (sum den_s)                     (the closed-form optimum of the (1 + S)-unknown problem);
// with one set both modes are the same chain bit for bit.
//
// Everything else is the chain of chain_body.inc — draw order (N·P at an attempt's start, P per step, retries going on in the
// stream), round-robin index, ft + (new - old), clip and generator transforms, start_from_minimum, the stop word, Philox keyed by
// rep_offset + rep — and with one set the sums, X and chi² are the numbers of chain_wave_kernel<M, QPL, true, false>.  How the chain
// draws is the text every family shares (chain_common.h: MCSAS_CHAIN_DRAWS, draw_value, MCSAS_INITIAL_ROW,
// MCSAS_PROPOSAL_ROW); the step, the fits and the outputs are this kernel's own: a hook or a template parameter in chain_body.inc
// changes every existing kernel's object.
//
// Layout: as chain_wave.h (q index i in lane i & 63, register slot i >> 6), and set s is padded to 64 k_s entries (pad: q of the
// set's first point, w = wI = I = 0), so that a register slot belongs to ONE set for the whole wave.  Bit j of SetsArgs::end_mask
// says that slot j is the last of its set.  Nothing per set is kept in registers, so nothing is indexed by a run-time set number
// (a register array so indexed goes to scratch): a lane sums into ONE running triple, and behind a set's last slot — a wave-uniform
// branch — the triple is reduced over the wave, meets the set's constants (a few doubles of LDS, indexed by the set counter: an
// argument block indexed at run time would be copied to scratch for it) and is folded into X_t; the triple starts again at zero.
// The live registers of the step are those of chain_wave_kernel plus X_t and the counter, both scalar.  The price is text: every
// slot carries a copy of the reduction and of the S_s - num²/den line (DESIGN §4.1e has the resource table).  The final scale,
// background and chi² of each set wait in LDS for the residual pass and for the one write of SetsOut at the end.
#pragma once
#include "chain_common.h"

namespace mcsas {

// what a chain reports per set
struct SetsOut { double scaling[MCSAS_MAX_SETS], background[MCSAS_MAX_SETS], chisq[MCSAS_MAX_SETS]; };

// what the comparison and the fits need of a set besides its sums: sum w, sum w I, sum w I² over its real points; 1 / Sw, SI / Sw and
// SII - SI² / Sw as chain_body.inc forms them (the host forms them with the same IEEE operations); its number of real points
struct SetConst { double Sw, SI, SII, invSw, SIoSw, Scen, nq; };

// The second kernel argument (as TraceArgs is the traced kernels'): ChainArgs stays what it is.  ChainArgs::nq is the number of real
// points of all sets, ChainArgs::qpad = 64 QPL covers the padded sets one after the other; ChainArgs::Sw / SI / SII are not read.
struct SetsArgs {
    int32_t  n_sets;                   // S, 1..MCSAS_MAX_SETS
    uint32_t end_mask;                 // bit j: register slot j is the last slot of its set (S bits are set)
    SetConst set[MCSAS_MAX_SETS];
    SetsOut *out;                      // [n_reps]
    int32_t  scale_mode, pad;          // MCSAS_SETS_SCALE_*: which instance the host launches (chain_sets_kernel<M, QPL, SHARED>); behind `out`: no earlier field moves
};
// in front of the wave kernels' LDS layout: each set's final scale, background and chi-squared, then its SetConst (as doubles),
// padded to 16 bytes
constexpr int SETS_CONST_DOUBLES = sizeof(SetConst) / sizeof(double);
constexpr int SETS_FIT_DOUBLES = 3;                        // a set's final scale, background and chi-squared
constexpr int SETS_LDS_DOUBLES = (SETS_FIT_DOUBLES * MCSAS_MAX_SETS + SETS_CONST_DOUBLES * MCSAS_MAX_SETS + 1) / 2 * 2;

// s1 = Σ w C, s2 = Σ w C², s3 = Σ w I C of one set (mcsas.py:376)
struct Sums3 { double s1, s2, s3; };

// set s's constants from where the kernel keeps them in LDS
static_assert(SETS_CONST_DOUBLES == 7, "set_const reads seven doubles");
__device__ __forceinline__ SetConst set_const(const double *lset, int s) {
    const double *c = lset + SETS_CONST_DOUBLES * s;
    return SetConst{c[0], c[1], c[2], c[3], c[4], c[5], c[6]};
}

// Walks this lane's slots of the intensity c and calls at_set(s, constants, sums) behind the last slot of set s with the set's sums
// over the wave (the same in every lane); wave-uniform throughout.
template <int QPL, class F>
__device__ __forceinline__ void sets_walk(const double (&c)[QPL], const double *lw, const double *lwI, const double *lset, int lane,
                                          uint32_t end_mask, F at_set) {
    Sums3 run{0., 0., 0.};
    int s = 0;
#pragma unroll
    for (int j = 0; j < QPL; ++j) {
        const double wt = lw[lane + WAVE * j] * c[j];
        run.s1 += wt; run.s2 = fma(wt, c[j], run.s2); run.s3 = fma(lwI[lane + WAVE * j], c[j], run.s3);
        if ((end_mask >> j) & 1u) {
            wave_sum3(run.s1, run.s2, run.s3);
            at_set(s, set_const(lset, s), run);
            ++s; run = Sums3{0., 0., 0.};
        }
    }
}

// the pieces of a set's chi²·Q_s at an optimum: S, num, den, centred sums when a background is fitted
struct SetParts { double S, num, den; };
__device__ __forceinline__ SetParts set_parts(bool find_bg, const SetConst &c, const Sums3 &s) {
    SetParts p{c.SII, s.s3, s.s2};
    if (find_bg) { p.S = c.Scen; p.num = fma(-c.SIoSw, s.s1, s.s3); p.den = fma(-(s.s1 * c.invSw), s.s1, s.s2); }
    return p;
}
// chi²·Q_s of a set at its own optimum: S - num²/den
__device__ __forceinline__ double set_x(bool find_bg, const SetConst &c, const Sums3 &s) {
    double S = c.SII, num = s.s3, den = s.s2;
    if (find_bg) { S = c.Scen; num = fma(-c.SIoSw, s.s1, s.s3); den = fma(-(s.s1 * c.invSw), s.s1, s.s2); }
    return S - num * num / den;
}

// the residual sum Σ w (I - A C - b)² of one set at (A, b), expanded in its sums
__device__ __forceinline__ double set_resid(const SetConst &c, const Sums3 &s, double A, double b) {
    const double SC = s.s1, SCC = s.s2, SIC = s.s3;
    return c.SII - 2. * A * SIC - 2. * b * c.SI + A * A * SCC + 2. * A * b * SC + b * b * c.Sw;
}

// argmin_{A,b} Σ w (I - A C - b)² of one set and the residual sum at that optimum: solve_fit (chain_common.h) without
// positive_background, on the set's own sums
__device__ __forceinline__ double set_fit(bool find_bg, const SetConst &c, const Sums3 &s, double &A, double &b) {
    const double SC = s.s1, SCC = s.s2, SIC = s.s3;
    if (find_bg) {
        const double det = c.Sw * SCC - SC * SC;
        A = (c.Sw * SIC - c.SI * SC) / det;
        b = (c.SI - A * SC) / c.Sw;
    } else {
        A = SIC / SCC; b = 0.;
    }
    return set_resid(c, s, A, b);
}

// MCSAS_SETS_SCALE_SHARED: ONE scale for all sets and a background per set, argmin over (A, b_0 .. b_{S-1}) of the residual sum over all
// points.  In: fit[3 s ..] = s1, s2, s3 of set s (LDS, where the walk left them).  Out: fit[3 s] = A = Σ num_s / Σ den_s,
// fit[3 s + 1] = b_s = (SI_s - A s1_s) / Sw_s (0 without a background); returns the sum of the sets' residual sums there.  With one set
// the pair is that set's own optimum by set_fit's operations: the one-set chain is the per-set mode's bit for bit.  Wave-uniform; the
// sets are walked through LDS, nothing per set is held in registers.
__device__ __forceinline__ double sets_fit_shared(bool find_bg, int n_sets, double *fit, const double *lset) {
    if (n_sets == 1) {
        const Sums3 s{fit[0], fit[1], fit[2]};
        double A, b;
        const double X = set_fit(find_bg, set_const(lset, 0), s, A, b);
        fit[0] = A; fit[1] = b;
        return X;
    }
    double Num = 0., Den = 0.;
    for (int s = 0; s < n_sets; ++s) {
        const double *f = fit + SETS_FIT_DOUBLES * s;
        const SetParts p = set_parts(find_bg, set_const(lset, s), Sums3{f[0], f[1], f[2]});
        Num += p.num; Den += p.den;
    }
    const double A = Num / Den;
    double X = 0.;
    for (int s = 0; s < n_sets; ++s) {
        double *f = fit + SETS_FIT_DOUBLES * s;
        const SetConst c = set_const(lset, s);
        const Sums3 sums{f[0], f[1], f[2]};
        const double b = find_bg ? (c.SI - A * sums.s1) / c.Sw : 0.;
        X += set_resid(c, sums, A, b);
        f[0] = A; f[1] = b;
    }
    return X;
}

#define MCSAS_SETS_MIN_WAVES(QPL) ((QPL) <= 8 ? 2 : 1)     // (chain_wave.h's, with cached rows)

// The chain of both scale modes, one wavefront: SHARED says how the sets' pieces meet in X_t and what the fits solve.
// chain_sets_kernel<M, QPL> is the MCSAS_SETS_SCALE_PER_SET instance (kern_wave_sets.hip), chain_sets_kernel<M, QPL, true> the
// MCSAS_SETS_SCALE_SHARED one (kern_wave_sets_shared.hip).  The kernel itself carries the text: handed on to a function, the argument
// blocks reach it another way and the per-set instances' registers and scratch move (the table of DESIGN §4.1e).
template <int M, int QPL, bool SHARED = false>
__global__ __launch_bounds__(64, MCSAS_SETS_MIN_WAVES(QPL)) void chain_sets_kernel(const ChainArgs a, const SetsArgs sa) {
    extern __shared__ double lds[];
    const int lane = threadIdx.x;
    const int rep = blockIdx.x;
    const int N = a.n_contrib, P = a.model.n_active, qpad = a.qpad;
    double *lfit = lds, *lq = lds + SETS_LDS_DOUBLES, *lw = lq + qpad, *lwI = lq + 2 * qpad, *lq3 = lq + 3 * qpad, *tab = lq + 4 * qpad;
    for (int i = lane; i < qpad; i += WAVE) {
        const double qq = a.q[i];
        lq[i] = qq; lw[i] = a.w[i]; lwI[i] = a.wI[i]; lq3[i] = 1.0 / (qq * qq * qq);
    }
    double *lset = lds + SETS_FIT_DOUBLES * MCSAS_MAX_SETS;
    if (lane == 0) {
#pragma unroll
        for (int s = 0; s < MCSAS_MAX_SETS; ++s) {
            double *c = lset + SETS_CONST_DOUBLES * s;
            c[0] = sa.set[s].Sw; c[1] = sa.set[s].SI; c[2] = sa.set[s].SII; c[3] = sa.set[s].invSw; c[4] = sa.set[s].SIoSw;
            c[5] = sa.set[s].Scen; c[6] = sa.set[s].nq;
        }
    }
    const QTables qt = make_qtables<M>(a.model, lq, lq3, tab);
    Contrib<M>::fill_table(a.model, tab, lane, WAVE);
    __syncthreads();

    const uint32_t end_mask = sa.end_mask;
    const bool find_bg = a.find_bg != 0;

    double *rset = a.rset + (size_t)rep * N * P;
    double *cache = a.cache + (size_t)rep * a.cache_rows * qpad;
    DrawSource src MCSAS_CHAIN_DRAWS(a, rep);
    int overflow = 0;
    uint64_t draw_pos = 0;                 // uniforms consumed so far by this rep (all attempts)
    const uint64_t t_start = wall_clock64();

    double ft[QPL];
    double chi2 = 0.;
    int64_t num_iter = 0, num_moves = 0, total_steps = 0;
    int attempts = 0, converged = 0, stopped = 0;
    const double nqd = (double)a.nq;

    for (int attempt = 0; attempt <= a.max_retries; ++attempt) {
        ++attempts;
        // ------------------------------------------------------------ initial parameter set (scatteringmodel.py:117-127)
#pragma unroll
        for (int j = 0; j < QPL; ++j) ft[j] = 0.;
        for (int n0 = 0; n0 < N; n0 += WAVE) {
            const int n = n0 + lane;
            double row[MCSAS_MAX_ACTIVE] = {0., 0., 0., 0.};
            MCSAS_INITIAL_ROW(row, n, n < N, false, true, draw_pos, overflow)
            Contrib<M> mine;
            mine.prepare(a.model, row);
            // model.calc(data, rset, c): rows accumulated in contribution order (scatteringmodel.py:90-101)
            const int cnt = min(WAVE, N - n0);
            for (int i = 0; i < cnt; ++i) {
                const Contrib<M> c = mine.bcast(__builtin_amdgcn_readfirstlane(i));
                double it[QPL];
                RowEval<M, QPL>::run(c, qt, lane, it);
#pragma unroll
                for (int j = 0; j < QPL; ++j) {
                    ft[j] += it[j];
                    cache[(size_t)(n0 + i) * qpad + lane + WAVE * j] = it[j];
                }
            }
        }
        if (!a.start_from_min) draw_pos += (uint64_t)N * P;

        // ------------------------------------------------------------ initial fit (mcsas.py:327-343), set by set
        double X = 0.;
        sets_walk<QPL>(ft, lw, lwI, lset, lane, end_mask, [&](int s, const SetConst &c, const Sums3 &sums) {
            if constexpr (SHARED) {                                                            // (the sums wait in LDS for sets_fit_shared)
                lfit[SETS_FIT_DOUBLES * s] = sums.s1; lfit[SETS_FIT_DOUBLES * s + 1] = sums.s2; lfit[SETS_FIT_DOUBLES * s + 2] = sums.s3;
            } else {
                double A, b;
                X += set_fit(find_bg, c, sums, A, b);
            }
        });
        if constexpr (SHARED) {
            X = sets_fit_shared(find_bg, sa.n_sets, lfit, lset);
            // Σ S_s in set order does not depend on the step: taken once per attempt and kept in set 0's chi² word, which is free until
            // the final fit (a register held across the row evaluation costs the integral models scratch)
            double Ssum = 0.;
            for (int s = 0; s < sa.n_sets; ++s) { const SetConst c = set_const(lset, s); Ssum += find_bg ? c.Scen : c.SII; }
            lfit[2] = Ssum;
        }
        chi2 = X / nqd;
        X = chi2 * nqd;
        num_iter = 0; num_moves = 0;
        int ri = 0;

        // ------------------------------------------------------------ MC loop (mcsas.py:354-404)
        bool running = (N > 1);
        while (running) {
            if (!(chi2 > a.conv_crit) || !(num_iter < a.max_iter)) break;
            if (stop_requested(a)) { stopped = 1; break; }
            // proposals for the next 64 steps, one per lane: P uniforms per step in parameter order (mcsas.py:358)
            double prow[MCSAS_MAX_ACTIVE] = {0., 0., 0., 0.};
            int povf = 0;
            MCSAS_PROPOSAL_ROW(prow, draw_pos + (uint64_t)(num_iter + lane) * P, num_iter + lane < a.max_iter, povf)
            Contrib<M> prop;
            prop.prepare(a.model, prow);

            for (int k = 0; k < WAVE; ++k) {
                if (!(chi2 > a.conv_crit) || !(num_iter < a.max_iter)) { running = false; break; }
                const int kk = __builtin_amdgcn_readfirstlane(k);
                const Contrib<M> cnew = prop.bcast(kk);
                if (__builtin_amdgcn_readlane(povf, kk)) overflow = 1;
                double inew[QPL], test[QPL];
                const double *orow = cache + (size_t)ri * qpad + lane;
#pragma unroll
                for (int j = 0; j < QPL; ++j) test[j] = orow[WAVE * j];
                RowEval<M, QPL>::run(cnew, qt, lane, inew);
                // (ft + (new - old) as in every execution mode, chain_body.inc; the walk of sets_walk with the candidate formed on the way)
                double Xt = 0.;
                {
                    [[maybe_unused]] double Num = 0., Den = 0.;                        // (SHARED: the sets' pieces in set order)
                    Sums3 run{0., 0., 0.};
                    int s = 0;
#pragma unroll
                    for (int j = 0; j < QPL; ++j) {
                        test[j] = ft[j] + (inew[j] - test[j]);
                        const double wt = lw[lane + WAVE * j] * test[j];
                        run.s1 += wt; run.s2 = fma(wt, test[j], run.s2); run.s3 = fma(lwI[lane + WAVE * j], test[j], run.s3);
                        if ((end_mask >> j) & 1u) {
                            wave_sum3(run.s1, run.s2, run.s3);
                            if constexpr (SHARED) {
                                const SetParts p = set_parts(find_bg, set_const(lset, s), run);
                                Num += p.num; Den += p.den;
                            } else {
                                Xt += set_x(find_bg, set_const(lset, s), run);
                            }
                            ++s; run = Sums3{0., 0., 0.};
                        }
                    }
                    if constexpr (SHARED) Xt = lfit[2] - Num * Num / Den;
                }
                if (Xt < X) {                                                          // mcsas.py:379-390
                    X = Xt;
                    chi2 = X / nqd;
#pragma unroll
                    for (int j = 0; j < QPL; ++j) {
                        ft[j] = test[j];
                        cache[(size_t)ri * qpad + lane + WAVE * j] = inew[j];
                    }
#pragma unroll
                    for (int p = 0; p < MCSAS_MAX_ACTIVE; ++p)
                        if (p < P) {
                            double val = readlane_f64(prow[p], kk);
                            if (lane == 0) rset[(size_t)ri * P + p] = val;
                        }
                    ++num_moves;
                }
                ri = (ri + 1 == N) ? 0 : ri + 1;                                       // mcsas.py:403-404
                ++num_iter;
            }
        }
        draw_pos += (uint64_t)num_iter * P;
        total_steps += num_iter;

        // ------------------------------------------------------------ final fit on ft (mcsas.py:424-426), set by set
        sets_walk<QPL>(ft, lw, lwI, lset, lane, end_mask, [&](int s, const SetConst &c, const Sums3 &sums) {
            if constexpr (SHARED) {
                lfit[SETS_FIT_DOUBLES * s] = sums.s1; lfit[SETS_FIT_DOUBLES * s + 1] = sums.s2; lfit[SETS_FIT_DOUBLES * s + 2] = sums.s3;
            } else {
                double A, b;
                (void)set_fit(find_bg, c, sums, A, b);
                lfit[SETS_FIT_DOUBLES * s] = A; lfit[SETS_FIT_DOUBLES * s + 1] = b;
            }
        });
        if constexpr (SHARED) (void)sets_fit_shared(find_bg, sa.n_sets, lfit, lset);
        // (every lane wrote each set's pair itself: its own reads below follow in program order)
        // reported chi-squared: direct residual sums, like chiSqr (backgroundscalingfit.py:72-77), each slot with its own set's fit;
        // the fit itself goes out on the way (ifinal*sc[0]+sc[1], mcsas.py:430: the last attempt's stays)
        {
            double all = 0., run = 0.;
            int s = 0;
            double cA = lfit[0], cb = lfit[1];
#pragma unroll
            for (int j = 0; j < QPL; ++j) {
                const double f = ft[j] * cA + cb;
                a.fit[(size_t)rep * qpad + lane + WAVE * j] = f;
                const double r = a.I[lane + WAVE * j] - f;
                run += lw[lane + WAVE * j] * r * r;
                if ((end_mask >> j) & 1u) {
                    const double v = wave_sum(run);
                    all += v;
                    lfit[SETS_FIT_DOUBLES * s + 2] = v / set_const(lset, s).nq;
                    ++s; run = 0.;
                    if (s < sa.n_sets) { cA = lfit[SETS_FIT_DOUBLES * s]; cb = lfit[SETS_FIT_DOUBLES * s + 1]; }   // (behind the last set: padding of weight zero)
                }
            }
            chi2 = all / nqd;
        }
        converged = !(chi2 > a.conv_crit);
        if (converged || stopped) break;
    }

    // ---------------------------------------------------------------- outputs (mcsas.py:428-439)
    overflow = __any(overflow);
    if (lane == 0) {
        ChainOut o;
        o.chisq = chi2; o.scaling = lfit[0]; o.background = lfit[1];  // set 0's
        o.seconds = (double)(wall_clock64() - t_start) * 1e-8;                    // 100 MHz counter
        o.num_iter = num_iter; o.num_moves = num_moves; o.draws = (int64_t)draw_pos;
        o.total_steps = total_steps;
        o.attempts = attempts; o.converged = converged; o.stream_overflow = overflow; o.stopped = stopped;
        a.out[rep] = o;
        SetsOut so;
#pragma unroll
        for (int s = 0; s < MCSAS_MAX_SETS; ++s) {
            const bool on = s < sa.n_sets;
            so.scaling[s] = on ? lfit[SETS_FIT_DOUBLES * s] : 0.; so.background[s] = on ? lfit[SETS_FIT_DOUBLES * s + 1] : 0.;
            so.chisq[s] = on ? lfit[SETS_FIT_DOUBLES * s + 2] : 0.;
        }
        sa.out[rep] = so;
    }
}

}  // namespace mcsas
