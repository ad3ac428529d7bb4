// chain_body.inc — one Monte-Carlo chain with the running intensity ft in registers (McSAS.mcFit, mcsas.py:287-439; retry loop
// of McSAS.analyse, :220-246), from its rset pointer to its ChainOut record: initial set, initial fit, batches of 64 proposals,
// the division-free comparison, the accept bookkeeping, retries, final fit.  Included verbatim, inside the kernel, by the
// wavefront-per-chain kernels (chain_wave_kernel.inc) and by the q-split workgroup kernel (chain_wide.h), so that both families
// compile from one text and a change to the step is made once.  Text, not a function or a policy object: either was measured to
// change the kernels' code (DESIGN §4.1a).
//
// In scope at the point of inclusion: M, QPL (template parameters); CACHE (compile-time bool: per-contribution rows are kept in
// a.cache; false re-evaluates the old row and folds the cache away) and GIVEN (compile-time bool: the first attempt takes the set
// the host left in rset instead of generating one, mcsas_hip_plan_set_start; false folds away); `const ChainArgs &a` (the
// analysis), `const int rep` (its repetition), `const int lane` (0..63), `N`, `P`, `qpad` (a.n_contrib, a.model.n_active,
// a.qpad), `qt` (the QTables of this lane's q-points: RowEval fills slot j of a lane with one of them) — and the hooks below.
// A hook is a macro the including file defines ahead of the #include and #undef's after it; the ones marked (text) stand for
// exactly the tokens given, without parentheses of their own, because the sums they are part of keep their order of evaluation.
//   CHAIN_STATE        declarations: what the sums below keep from one call to the next, if anything (it sits among the chain's own
//                      state because moving a declaration was measured to change the code)
//   CHAIN_CACHE_PTR(p) where this thread's `cache` pointer starts, given the repetition's first row p
//   CHAIN_ROW(r)       (text) offset from `cache` of this lane's slot 0 in row r; slot j is WAVE * j further
//   CHAIN_Q(j)         (text) index of this lane's slot j into the padded data (a.I, one row of a.fit)
//   CHAIN_W(j)         w = 1/sigma^2 at slot j
//   CHAIN_WI(j)        wI = I/sigma^2 at slot j
//   CHAIN_SUM3(x,y,z)  statement: replaces three per-lane values by their sums over the chain's q-points, the same in every thread
//   CHAIN_SUM1(x)      expression: that sum of one per-lane value
//   CHAIN_FIRST        true in one thread per lane index: those write the initial set to rset
//   CHAIN_LEADER       true in one thread of the chain: it writes an accepted row to rset, and the record
//   CHAIN_STOP         expression: McSAS.stop has been asked for — one answer for all threads of the chain
//   CHAIN_TRACE_START(c)          statement, or nothing: an attempt starts with reduced chi² c of its initial set (mcsas.py:343-344)
//   CHAIN_TRACE_MOVE(i, s, c, k)  statement, or nothing: move i of the attempt was accepted at step s and left reduced chi² c; its
//                      values are lane k of prow (mcsas.py:385-390).  Only the traced kernels (chain_wave.h, chain_wide.h) put anything here
    double *rset = a.rset + (size_t)rep * N * P;
    double *cache = CACHE ? CHAIN_CACHE_PTR(a.cache + (size_t)rep * a.cache_rows * qpad) : nullptr;
    DrawSource src MCSAS_CHAIN_DRAWS(a, rep);
    int overflow = 0;
    CHAIN_STATE
    uint64_t draw_pos = 0;                 // uniforms consumed so far by this rep (all attempts)
    const uint64_t t_start = wall_clock64();

    double ft[QPL];
    FitResult cur{1.0, 0.0, 0.0};
    int64_t num_iter = 0, num_moves = 0, total_steps = 0;
    int attempts = 0, converged = 0, stopped = 0;

    for (int attempt = 0; attempt <= a.max_retries; ++attempt) {
        ++attempts;
        // ------------------------------------------------------------ initial parameter set
        // generateParameters(N): N draws per active parameter, parameter-major (scatteringmodel.py:117-127); a given start
        // (GIVEN, first attempt only) stands in for it and consumes no draws
        const bool given = GIVEN && attempt == 0;
#pragma unroll
        for (int j = 0; j < QPL; ++j) ft[j] = 0.;
        for (int n0 = 0; n0 < N; n0 += WAVE) {
            const int n = n0 + lane;
            double row[MCSAS_MAX_ACTIVE] = {0., 0., 0., 0.};
            MCSAS_INITIAL_ROW(row, n, n < N, given, CHAIN_FIRST, draw_pos, overflow)
            Contrib<M> mine;                                       // (where a chain has several waves, each prepares all 64: the same numbers)
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
                    if (CACHE) cache[CHAIN_ROW(n0 + i) + WAVE * j] = it[j];
                }
            }
        }
        if (!given && !a.start_from_min) draw_pos += (uint64_t)N * P;

        // ------------------------------------------------------------ initial fit (mcsas.py:327-343)
        {
            double s1 = 0., s2 = 0., s3 = 0.;
#pragma unroll
            for (int j = 0; j < QPL; ++j) {
                double wt = CHAIN_W(j) * ft[j];
                s1 += wt; s2 = fma(wt, ft[j], s2); s3 = fma(CHAIN_WI(j), ft[j], s3);
            }
            CHAIN_SUM3(s1, s2, s3);
            cur = solve_fit(a, s1, s2, s3);
        }
        CHAIN_TRACE_START(cur.chi2)
        num_iter = 0; num_moves = 0;
        int ri = 0;
        // The comparison chi²_t < chi² (mcsas.py:379) is made without divisions, as in the other kernels:
        // chi²·Q = S - num²/den at the optimum (centred sums when a background is fitted), so
        // chi²_t < chi²  <=>  num² > (S - X) den  with X = chi²·Q of the current state; the one division is
        // paid when a move is accepted.  Scale and background are only needed at the end of the attempt.
        const double nqd = (double)a.nq, invSw = 1.0 / a.Sw, SIoSw = a.SI / a.Sw, Scen = a.SII - a.SI * a.SI / a.Sw;
        double X = cur.chi2 * nqd;

        // ------------------------------------------------------------ MC loop (mcsas.py:354-404)
        bool running = (N > 1);
        while (running) {
            if (!(cur.chi2 > a.conv_crit) || !(num_iter < a.max_iter)) break;
            if (CHAIN_STOP) { stopped = 1; break; }
            // proposals for the next 64 steps, one per lane (the same in every wave of the chain): generateParameters() draws
            // P uniforms per step in parameter order (mcsas.py:358)
            double prow[MCSAS_MAX_ACTIVE] = {0., 0., 0., 0.};
            int povf = 0;
            MCSAS_PROPOSAL_ROW(prow, draw_pos + (uint64_t)(num_iter + lane) * P, num_iter + lane < a.max_iter, povf)
            Contrib<M> prop;
            prop.prepare(a.model, prow);

            int k = 0;
            for (; k < WAVE; ++k) {
                if (!(cur.chi2 > a.conv_crit) || !(num_iter < a.max_iter)) { running = false; break; }
                const int kk = __builtin_amdgcn_readfirstlane(k);
                const Contrib<M> cnew = prop.bcast(kk);
                if (__builtin_amdgcn_readlane(povf, kk)) overflow = 1;
                double inew[QPL], test[QPL];
                if (CACHE) {
                    const double *orow = cache + CHAIN_ROW(ri);
#pragma unroll
                    for (int j = 0; j < QPL; ++j) test[j] = orow[WAVE * j];
                } else {
                    // model.calc(data, rset[ri]) re-evaluated like mcsas.py:362
                    double orow[MCSAS_MAX_ACTIVE];
#pragma unroll
                    for (int p = 0; p < MCSAS_MAX_ACTIVE; ++p) orow[p] = (p < P) ? rset[(size_t)ri * P + p] : 0.;
                    Contrib<M> cold;
                    cold.prepare(a.model, orow);
                    RowEval<M, QPL>::run(cold, qt, lane, test);
                }
                double s1 = 0., s2 = 0., s3 = 0.;
                RowEval<M, QPL>::run(cnew, qt, lane, inew);
#pragma unroll
                for (int j = 0; j < QPL; ++j) {
                    // mcsas.py:367 has (ft - old) + new; every execution mode here adds the fp64 difference d = new - old
                    // instead (the workgroup and pipeline kernels carry d rows), so that ft is the SAME number in all
                    // three modes — at most one ulp per accepted move away from the reference's order
                    test[j] = ft[j] + (inew[j] - test[j]);
                    double wt = CHAIN_W(j) * test[j];
                    s1 += wt; s2 = fma(wt, test[j], s2); s3 = fma(CHAIN_WI(j), test[j], s3);
                }
                CHAIN_SUM3(s1, s2, s3);
                // s1 = Σ w C, s2 = Σ w C², s3 = Σ w I C of the candidate (mcsas.py:376)
                double S = a.SII, num = s3, den = s2;
                if (a.find_bg) {
                    const double numc = fma(-SIoSw, s1, s3), denc = fma(-(s1 * invSw), s1, s2);
                    const bool neg_b = a.pos_bg && (fma(a.SI, denc, -(numc * s1)) < 0.);
                    if (!neg_b) { S = Scen; num = numc; den = denc; }
                }
                if (num * num > (S - X) * den) {                                   // mcsas.py:379-390
                    X = S - num * num / den;
                    cur.chi2 = X / nqd;
#pragma unroll
                    for (int j = 0; j < QPL; ++j) {
                        ft[j] = test[j];
                        if (CACHE) cache[CHAIN_ROW(ri) + WAVE * j] = inew[j];
                    }
#pragma unroll
                    for (int p = 0; p < MCSAS_MAX_ACTIVE; ++p)
                        if (p < P) {
                            double val = readlane_f64(prow[p], kk);
                            if (CHAIN_LEADER) rset[(size_t)ri * P + p] = val;
                        }
                    if (!CACHE) __threadfence_block();   // rset[ri] is re-read by every lane N steps later
                    CHAIN_TRACE_MOVE(num_moves, num_iter, cur.chi2, kk)
                    ++num_moves;
                }
                ri = (ri + 1 == N) ? 0 : ri + 1;                                   // mcsas.py:403-404
                ++num_iter;
            }
        }
        draw_pos += (uint64_t)num_iter * P;
        total_steps += num_iter;

        // ------------------------------------------------------------ final fit on ft (mcsas.py:424-426)
        {
            double s1 = 0., s2 = 0., s3 = 0.;
#pragma unroll
            for (int j = 0; j < QPL; ++j) {
                double wt = CHAIN_W(j) * ft[j];
                s1 += wt; s2 = fma(wt, ft[j], s2); s3 = fma(CHAIN_WI(j), ft[j], s3);
            }
            CHAIN_SUM3(s1, s2, s3);
            cur = solve_fit(a, s1, s2, s3);
            // reported chi-squared: direct residual sum, like chiSqr (backgroundscalingfit.py:72-77)
            double rs = 0.;
#pragma unroll
            for (int j = 0; j < QPL; ++j) {
                double r = a.I[CHAIN_Q(j)] - (ft[j] * cur.A + cur.b);
                rs += CHAIN_W(j) * r * r;
            }
            cur.chi2 = CHAIN_SUM1(rs) / (double)a.nq;
        }
        converged = !(cur.chi2 > a.conv_crit);
        if (converged || stopped) break;
    }

    // ---------------------------------------------------------------- outputs (mcsas.py:428-439)
#pragma unroll
    for (int j = 0; j < QPL; ++j)
        a.fit[(size_t)rep * qpad + CHAIN_Q(j)] = ft[j] * cur.A + cur.b;           // ifinal*sc[0]+sc[1]
    overflow = __any(overflow);
    if (CHAIN_LEADER) {
        ChainOut o;
        o.chisq = cur.chi2; o.scaling = cur.A; o.background = cur.b;
        o.seconds = (double)(wall_clock64() - t_start) * 1e-8;                    // 100 MHz counter
        o.num_iter = num_iter; o.num_moves = num_moves; o.draws = (int64_t)draw_pos;
        o.total_steps = total_steps;
        o.attempts = attempts; o.converged = converged; o.stream_overflow = overflow; o.stopped = stopped;
        a.out[rep] = o;
    }
