// pipe_prod_overlap.inc — the overlapped variant of the producer's row loop (tuning word bit 18; pipe_geometry: overlap), a
// measurement build's.  Included once, inside pipe_prod_block (pipe_prod.h), whose locals it uses; kept as text because a
// function of its own would change the generated code.
        // Phase ss = the rows of sub-window ss, every wave its share.  The Gram block of sub-window ss - 1 is worked off
        // in units BETWEEN the rows of phase ss (matrix pipe beside the vector pipe: while one wave of a SIMD is inside a run
        // of MFMAs its partner has the vector issue slots to itself), its operands read back from the window buffer.
        // One barrier per phase, and it waits for no memory: a wave passes B(ss - 1) — "the rows of ss - 1 are visible to the
        // workgroup" — behind its FIRST row of phase ss, after a counted wait that covers exactly its stores of phase
        // ss - 1 (the counter is in order: everything older than that row's own stores has completed by then).  The partial
        // tiles of a block are parked in LDS when a wave has done its last unit and summed by all threads behind the next
        // barrier (two reduction buffers, by parity).  Only the last sub-window's Gram block runs with nothing beside it.
        // Rows per wave and sub-window, a fixed deal: W / 8 on average; tuning bits 19-20 shift rows from the four waves that
        // share their SIMDs with an older wave (4-7) to the older ones (0-3): 0 = equal shares, 1 / 2 = one / two rows.
        const int wv = __builtin_amdgcn_readfirstlane(wave);
        const int rw_even = W >> 3, skew_req = (MCSAS_TUNE_BITS(a) >> 19) & 3;
        const int skew = skew_req < rw_even ? skew_req : rw_even - 1;
        const int RW = wv < 4 ? rw_even + skew : rw_even - skew;                        // my rows per sub-window
        const int rbase = wv < 4 ? wv * (rw_even + skew) : 4 * (rw_even + skew) + (wv - 4) * (rw_even - skew);   // my first row in a sub-window
        constexpr size_t GRED = (size_t)PIPE_WAVES * PIPE_GRAM_NT_MAX * 256;
        const int nmine = nsb * RW;                                                    // my rows (<= 8), lane l <-> my l-th row
        const int lrow = (lane / RW) * W + rbase + (lane % RW);                        // its offset in the block
        // Lanes 32 + l of a wave mirror its lanes l: the same rows, their `old` side (see the stale rows in pipe_prod.h).
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
                    const double pv = draw_value(a, p, u);
                    if (!(old_lane && sb0 + ((l2 / RW) * W + rbase + (l2 % RW)) < max_iter)) prow[p] = pv;
                }
        }
        Contrib<M> prop;
        prop.prepare(a.model, prow);
        PIPE_TLX_MARK(pa, t, 1);
        if (stale_r >= 0) stale_push(stale_r, prop);
        if (lazy) stale_refresh();
        PIPE_TLX_MARK(pa, t, 2);
        PIPE_TLX_MARK(pa, t, 3);
        // proposals and replay-overflow flags of all my rows: one store per wave (lane l <-> my l-th row)
        if (lane < nmine) {
            const int k = by * BR + lrow;
#pragma unroll
            for (int p = 0; p < MCSAS_MAX_ACTIVE; ++p) if (p < P) pval[k * MCSAS_MAX_ACTIVE + p] = prow[p];
            povf[k] = pov;
        }
        const int ntiles = pipe_gram_tiles(W);
        constexpr int UN = QPL;                                   // Gram units (8 q each) of my q slice
        // the tile scheme is uniform for the launch; everything below is compiled once per scheme
        auto rows_and_gram = [&](auto scheme_t, auto scheme_pack) {
            constexpr int T = decltype(scheme_t)::value;
            constexpr bool PACK = decltype(scheme_pack)::value;
            constexpr int UCAP = PipeGramScheme<T, PACK>::UCAP;
            v4f64 gacc[PIPE_GRAM_NT_MAX];
            v2f64 G[PIPE_GRAM_PREF];
            for (int ss = 0; ss < nsb; ++ss) {
                const int nv_prev = ss > 0 ? nvalid_of(ss - 1) : 0;
                const bool gram_live = ss > 0 && !no_gram && nv_prev > 0;             // uniform in the block
                const auto dprev = dwin + (size_t)(by * BR + (ss > 0 ? ss - 1 : 0) * W) * qpad;
                for (int jr = 0; jr < RW; ++jr) {
                    const int l = ss * RW + jr, bl = __builtin_amdgcn_readfirstlane(l);
                    const int kl = ss * W + rbase + jr, k = by * BR + kl;
                    const Contrib<M> cnew = prop.bcast(bl);
                    const int sslot = __builtin_amdgcn_readlane(my_sslot, bl);
                    // the `old` row of THIS step is requested here and used behind the row evaluation, which is longer than the
                    // round trip (a row of lookahead would hold another QPL doubles per lane across the evaluation, beside the
                    // Gram operands and accumulators)
                    double d[QPL], nwv[QPL], ocur[QPL];
                    {
                        const auto orow = cache + (size_t)__builtin_amdgcn_readlane(my_oslot, bl) * qpad + lane;
#pragma unroll
                        for (int j = 0; j < QPL; ++j) ocur[j] = orow[WAVE * j];
                    }
                    // my units of block ss - 1 that go with this row (none with the first row of a phase: B(ss - 1) comes
                    // behind it): their operands are requested now and land while the row is evaluated
                    const int u0 = (RW > 1 && jr > 0) ? UN * (jr - 1) / (RW - 1) : 0, u1 = (RW > 1 && jr > 0) ? UN * jr / (RW - 1) : 0;
                    const int npre = u1 - u0 < UCAP ? u1 - u0 : UCAP;
                    const bool chunk = gram_live && npre > 0;                        // uniform in the wave
                    if (chunk) pipe_gram_fetch<QPL, T, PACK>(dprev, qpad, nv_prev, wv, u0, npre, G);
                    else {
#pragma unroll
                        for (int i = 0; i < PIPE_GRAM_PREF; ++i) asm volatile("" : "=v"(G[i]));   // (defined on both paths: no copy at the join)
                    }
                    // (a row behind max_iter — the last window of a run only — is evaluated like any other: its proposal is the
                    // generators' midpoint, its stores land in slots nobody reads, the Gram block masks it; no branch around the
                    // row means no join at which the compiler would wait for this row's stores)
                    const auto nrow = cache + (size_t)sslot * qpad + lane;
                    const auto dr = dwin + (size_t)k * qpad + lane;
                    RowEval<M, QPL>::run(cnew, qt, lane, nwv);
                    PIPE_PIN_ROW(ocur); PIPE_PIN_ROW(nwv);                        // the `old` row has landed before the first store is issued
                    if (chunk) {
                        pipe_gram_consume<QPL, T, PACK>(G, nv_prev, lw, wv, u0, npre, gacc);
                        if (u0 + npre < u1) pipe_gram_units<QPL, T, PACK>(dprev, qpad, nv_prev, lw, wv, u0 + npre, u1, gacc);
                        if (u1 == UN) pipe_gram_park(gacc, ntiles, gred + (size_t)((ss - 1) & 1) * GRED, wv, lane);
                    }
                    double s1 = 0., s2 = 0.;
#pragma unroll
                    for (int j = 0; j < QPL; ++j) {
                        const int iq = lane + WAVE * j;
                        if (!lazy) nrow[WAVE * j] = nwv[j];
                        d[j] = nwv[j] - ocur[j];
                        dr[WAVE * j] = d[j];
                        s1 = fma(lw[iq], d[j], s1); s2 = fma(lwI[iq], d[j], s2);
                    }
                    // a = sum w d (even lanes), e = sum wI d (odd lanes); g = sum w d^2 is the Gram block's diagonal
                    const double ae = wave_sum2_split(s1, s2, lane);
                    if (lane < 2) scal[(size_t)k * 4 + lane] = ae;
                    PIPE_TL_MARK(pa, t, (ss < 2 ? ss : 1) * 4 + (jr < 3 ? jr : 3));
                    if (ss > 0 && !no_gram && jr == 0) {
                        // B(ss - 1): my stores of phase ss - 1 are older than this row's QPL (or more) stores
                        asm volatile("s_waitcnt vmcnt(%0)" :: "n"(QPL < 8 ? QPL : 8) : "memory");
                        PIPE_LDS_BARRIER();
                        if (ss > 1 && nvalid_of(ss - 2) > 0)                          // every wave's tiles of block ss - 2 are parked: sum them
                            pipe_gram_sum_store(W, gred + (size_t)((ss - 2) & 1) * GRED, gwin + (size_t)(by * nsb + ss - 2) * W * W,
                                                scal + (size_t)(by * BR + (ss - 2) * W) * 4);
                        if (RW == 1 && nv_prev > 0) {                                 // one row per wave and phase: nothing to put the units beside
                            pipe_gram_units<QPL, T, PACK>(dprev, qpad, nv_prev, lw, wv, 0, UN, gacc);
                            pipe_gram_park(gacc, ntiles, gred + (size_t)((ss - 1) & 1) * GRED, wv, lane);
                        }
                    }
                }
                PIPE_TL_MARK(pa, t, 8 + (ss < 3 ? ss : 3));
            }
            // ---- the tail: block nsb - 2 is summed, the last sub-window's Gram block has nothing to run beside
            if (!no_gram) {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                PIPE_TL_MARK(pa, t, 12);
                PIPE_LDS_BARRIER();                                   // B(nsb - 1)
                PIPE_TL_MARK(pa, t, 13);
                if (nsb > 1 && nvalid_of(nsb - 2) > 0)
                    pipe_gram_sum_store(W, gred + (size_t)((nsb - 2) & 1) * GRED, gwin + (size_t)(by * nsb + nsb - 2) * W * W,
                                        scal + (size_t)(by * BR + (nsb - 2) * W) * 4);
                const int nv = nvalid_of(nsb - 1);
                if (nv > 0) {                                         // uniform in the block
                    const auto dlast = dwin + (size_t)(by * BR + (nsb - 1) * W) * qpad;
                    // batches of UCAP units, the next batch's operands requested before this one's MFMAs
                    v2f64 G2[PIPE_GRAM_PREF];
                    PIPE_TL_MARK(pa, t, 14);
                    pipe_gram_fetch<QPL, T, PACK>(dlast, qpad, nv, wv, 0, UN < UCAP ? UN : UCAP, G);
                    for (int u = 0; u < UN; u += 2 * UCAP) {
                        const int n0 = UN - u < UCAP ? UN - u : UCAP;
                        const int un = u + UCAP, n1 = un < UN ? (UN - un < UCAP ? UN - un : UCAP) : 0;
                        if (n1 > 0) pipe_gram_fetch<QPL, T, PACK>(dlast, qpad, nv, wv, un, n1, G2);
                        pipe_gram_consume<QPL, T, PACK>(G, nv, lw, wv, u, n0, gacc);
                        const int u2 = u + 2 * UCAP, n2 = u2 < UN ? (UN - u2 < UCAP ? UN - u2 : UCAP) : 0;
                        if (n2 > 0) pipe_gram_fetch<QPL, T, PACK>(dlast, qpad, nv, wv, u2, n2, G);
                        if (n1 > 0) pipe_gram_consume<QPL, T, PACK>(G2, nv, lw, wv, un, n1, gacc);
                    }
                    PIPE_TL_MARK(pa, t, 15);
                    pipe_gram_park(gacc, ntiles, gred + (size_t)((nsb - 1) & 1) * GRED, wv, lane);
                    PIPE_LDS_BARRIER();
                    PIPE_TL_MARK(pa, t, 16);
                    pipe_gram_sum_store(W, gred + (size_t)((nsb - 1) & 1) * GRED, gwin + (size_t)(by * nsb + nsb - 1) * W * W,
                                        scal + (size_t)(by * BR + (nsb - 1) * W) * 4);
                }
            }
        };
        if (W == 24) rows_and_gram(std::integral_constant<int, 2>{}, std::integral_constant<bool, true>{});
        else if (W <= 16) rows_and_gram(std::integral_constant<int, 1>{}, std::integral_constant<bool, false>{});
        else rows_and_gram(std::integral_constant<int, 2>{}, std::integral_constant<bool, false>{});
