// pipe_gram.h — the Gram block of a sub-window on the producer blocks of the pipeline (chain_pipe.h), fp64 MFMA.  The release
// path reads its operands from the LDS copy of the rows (pipe_prod_gram_lds); a tuning build adds the family that the overlapped
// producer (pipe_prod_overlap.inc) issues in units between its rows, operands from HBM/L2.
#pragma once
#include "pipe_layout.h"

namespace mcsas {

// Workgroup barrier for data handed over through LDS only: wait for this wave's LDS traffic, not for its global
// loads and stores.  __syncthreads() also drains vmcnt — in the scan loop that would make every barrier wait
// for the row batch that was prefetched just before it and for the stores of the accepted rows (a memory round
// trip per barrier).  The "memory" clobbers keep the compiler from moving LDS accesses across (the barrier
// builtin itself is IntrNoMem).
#define PIPE_LDS_BARRIER() do { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); __builtin_amdgcn_s_barrier(); asm volatile("" ::: "memory"); } while (0)

typedef double v4f64 __attribute__((ext_vector_type(4)));
typedef double v2f64 __attribute__((ext_vector_type(2)));

// ------------------------------------------------------------------------------------ producer
// Gram block of one sub-window, G[a][k] = Σ_q w_q d_a(q) d_k(q) over the W rows this block has just evaluated,
// with v_mfma_f64_16x16x4_f64: D(16x16) += A(16x4) B(4x16), lane l supplies A[l % 16][l / 16] and
// B[l / 16][l % 16], result register r holds D[4 r + l / 16][l % 16].  With A = d rows and B = (w d) rows both
// operands of lane l are the SAME element (row l % 16, q-slot l / 16) — one load, one multiply, one MFMA.
// The q range is cut into eight slices, slice v = [v 8 QPL, (v + 1) 8 QPL), each summed for ALL tiles into a partial of
// its own (which waves take them: pipe_prod_gram_lds_t); one operand load covers 8 consecutive q of the slice, two per
// lane slot kk = l / 16 (any assignment of q to MFMA k-slots is fine, the sum runs over all of them).
// The eight partial tiles are then summed in slice order through LDS (deterministic) and written to
// gout[a][k], a, k < W.

// tile number -> (row group, column group) of the upper triangle, and the store of one summed element
template <int T>
__device__ __forceinline__ void pipe_gram_store(int tsel, int idx, double sum, int W, MCSAS_GLOBAL double *gout, MCSAS_GLOBAL double *scal_sub = nullptr) {
    int ti = 0, tgi = 0, tgj = 0;
#pragma unroll
    for (int gi = 0; gi < T; ++gi)
#pragma unroll
        for (int gj = gi; gj < T; ++gj) { if (ti == tsel) { tgi = gi; tgj = gj; } ++ti; }
    const int i = 4 * (idx >> 6) + ((idx & 63) >> 4), j = idx & 15;   // result register r of lane l holds D[4 r + l / 16][l % 16]
    const int ar = 16 * tgi + i, kc = 16 * tgj + j;
    if (ar < W && kc < W) {
        gout[(size_t)ar * W + kc] = sum;
        if (scal_sub && ar == kc) scal_sub[ar * 4 + 2] = sum;
    }
}

// The operands are read from the LDS copy of the sub-window's d rows (row stride dstr).  T = 16-row groups of the
// sub-window (1..4), compile time: straight-line MFMA code.
// PACK (W = 24, three 8-row groups g0 g1 g2): the six upper-triangular 8x8 blocks fit TWO 16x16 tiles instead of the
// three of the 16-row grouping — tile 0 = rows [g0 g1] x columns [g1 g2] (blocks 01 02 11 12), tile 1 = rows and
// columns [g0 g2] (blocks 00 22; its 02 is a duplicate and not stored): a third fewer MFMAs.
// One call takes the tiles [R0, R0 + RN) of the sub-window's NT (a round of the reduction) for NS slices, gw and (NS = 2) gw + 4,
// each slice into an accumulator set of its own: every tile of a slice is accumulated over the slice in the same order whichever
// call takes it.  The operands of the next 8 q are requested in front of the MFMAs of the current ones (pinned by the scheduling
// barrier): one wave has to cover its own LDS latency — the partner wave of its SIMD, which used to, is not in here — and the
// MFMAs of the two slices alternate, four independent accumulator chains.
// FULL: every row an operand is read from is a valid row of the sub-window (nvalid == W and the row groups end at W: every
// window but a run's last) — no clamp of the row and no select per operand (two v_cndmask per double, three operands, every
// step); the values that reach the MFMAs are the ones the masked form lets through, so the bits are the same.
template <int QPL, int T, bool PACK, int R0, int RN, int NS, bool FULL>
__device__ __forceinline__ void pipe_gram_mfma_lds(const double *drows, int dstr, int nvalid, const double *lw, int gw, v4f64 (&acc)[NS][RN]) {
    const int lane = threadIdx.x & 63;
    const int m = lane & 15, kk = lane >> 4;
    constexpr int NT = PACK ? 2 : T * (T + 1) / 2;
    constexpr int NL = PACK ? 3 : T;                          // row operands per lane, slice and step-pair
    constexpr int SLICE = 64 * QPL / PIPE_WAVES, STEPS = SLICE / 8;
    constexpr int SSTR = (PIPE_WAVES / 2) * SLICE;            // from slice gw to slice gw + 4
    static_assert(SLICE >= 8, "too many waves for this q count");
    static_assert(R0 >= 0 && RN >= 1 && R0 + RN <= NT && (!PACK || (R0 == 0 && RN == 2)) && (NS == 1 || NS == 2), "tiles and slices of the sub-window");
    const int qs = gw * SLICE + kk * 2;
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
        for (int i = 0; i < RN; ++i) acc[s][i] = (v4f64){0., 0., 0., 0.};
    const double *rowp[NL];
    bool rowok[NL];
#pragma unroll
    for (int gi = 0; gi < NL; ++gi) {
        const int rr = PACK ? (gi == 0 ? m : gi == 1 ? 8 + m : (m < 8 ? m : m + 8)) : 16 * gi + m;
        rowok[gi] = FULL || rr < nvalid;
        rowp[gi] = drows + (size_t)(rowok[gi] ? rr : 0) * dstr + qs;
    }
    auto fetch = [&](int sp, v2f64 (&x)[NS][NL], v2f64 (&wv)[NS]) {
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            wv[s] = *reinterpret_cast<const v2f64 *>(lw + qs + s * SSTR + 8 * sp);
#pragma unroll
            for (int gi = 0; gi < NL; ++gi) x[s][gi] = *reinterpret_cast<const v2f64 *>(rowp[gi] + s * SSTR + 8 * sp);   // (a row group no tile of this call needs is not loaded: dead code)
        }
    };
    v2f64 cur[NS][NL], cw[NS];
    fetch(0, cur, cw);
#pragma unroll
    for (int sp = 0; sp < STEPS; ++sp) {
        v2f64 nxt[NS][NL], nw[NS];
        if (sp + 1 < STEPS) fetch(sp + 1, nxt, nw);
        __builtin_amdgcn_sched_barrier(0);
        v2f64 av[NS][NL], bv[NS][NL];
#pragma unroll
        for (int s = 0; s < NS; ++s)
#pragma unroll
            for (int gi = 0; gi < NL; ++gi) {
                if constexpr (FULL) av[s][gi] = cur[s][gi];
                else av[s][gi] = rowok[gi] ? cur[s][gi] : (v2f64){0., 0.};
                bv[s][gi] = av[s][gi] * cw[s];
            }
        if constexpr (PACK) {
#pragma unroll
            for (int s = 0; s < NS; ++s) acc[s][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[s][0].x, bv[s][1].x, acc[s][0], 0, 0, 0);
#pragma unroll
            for (int s = 0; s < NS; ++s) acc[s][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[s][2].x, bv[s][2].x, acc[s][1], 0, 0, 0);
#pragma unroll
            for (int s = 0; s < NS; ++s) acc[s][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[s][0].y, bv[s][1].y, acc[s][0], 0, 0, 0);
#pragma unroll
            for (int s = 0; s < NS; ++s) acc[s][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[s][2].y, bv[s][2].y, acc[s][1], 0, 0, 0);
        } else {
            int ti = 0;
#pragma unroll
            for (int gi = 0; gi < T; ++gi)
#pragma unroll
                for (int gj = gi; gj < T; ++gj) {
                    if (ti >= R0 && ti < R0 + RN) {
#pragma unroll
                        for (int s = 0; s < NS; ++s) acc[s][ti - R0] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[s][gi].x, bv[s][gj].x, acc[s][ti - R0], 0, 0, 0);
#pragma unroll
                        for (int s = 0; s < NS; ++s) acc[s][ti - R0] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[s][gi].y, bv[s][gj].y, acc[s][ti - R0], 0, 0, 0);
                    }
                    ++ti;
                }
        }
        if (sp + 1 < STEPS) {
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                cw[s] = nw[s];
#pragma unroll
                for (int gi = 0; gi < NL; ++gi) cur[s][gi] = nxt[s][gi];
            }
        }
    }
}

// element idx of packed tile tsel -> (row, column) of the 24-step sub-window, or skipped
// (the block's diagonal, g_k = sum_q w d_k^2, is the third of a step's ft-independent sums: to scal_sub[k][2])
__device__ __forceinline__ void pipe_gram_store_pack(int tsel, int idx, double sum, MCSAS_GLOBAL double *gout, MCSAS_GLOBAL double *scal_sub) {
    const int i = 4 * (idx >> 6) + ((idx & 63) >> 4), j = idx & 15;
    if (tsel == 0) {
        gout[(size_t)i * 24 + 8 + j] = sum;
        if (i == 8 + j) scal_sub[i * 4 + 2] = sum;
    } else if ((i < 8) == (j < 8)) {
        const int ar = i < 8 ? i : i + 8, kc = j < 8 ? j : j + 8;
        gout[(size_t)ar * 24 + kc] = sum;
        if (ar == kc) scal_sub[ar * 4 + 2] = sum;
    }
}

// a matrix wave's share of a round: the partial tiles of its NS slices, wave and (NS = 2) wave + 4, into their slots of gred
template <int QPL, int T, bool PACK, int R0, int RN, int NS, bool FULL>
__device__ __forceinline__ void pipe_gram_partials(const double *drows, int dstr, int nvalid, const double *lw, double *gred, int wave) {
    const int lane = threadIdx.x & 63;
    constexpr int TPR = PIPE_GRAM_TILES_PER_ROUND;
    v4f64 acc[NS][RN];
    pipe_gram_mfma_lds<QPL, T, PACK, R0, RN, NS, FULL>(drows, dstr, nvalid, lw, wave, acc);
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
        for (int u = 0; u < RN; ++u)
#pragma unroll
            for (int r = 0; r < 4; ++r) gred[((size_t)((wave + s * (PIPE_WAVES / 2)) * TPR + u) * 4 + r) * 64 + lane] = acc[s][u][r];
}

// Roles (`split`: a sub-window whose successor in the block lends the row waves a row, pipe_prod.h): only the MATRIX waves 0-3 —
// one per SIMD, the older of each pair, whose few operand multiplies win the vector arbitration — issue the MFMAs: wave v takes
// the two q slices that waves v and v + 4 take with eight Gram waves, each in an accumulator set of its own, in the same order,
// to the same partial slots v and v + 4 of gred; the sum over the eight partials and the store are unchanged, so the block comes
// out bit for bit the same.  The matrix pipe of a SIMD sees the same MFMAs either way; its vector pipe is free for the ROW waves
// 4-7, which come here late (from a row of the next sub-window, evaluated beside the first MFMAs), issue none, and call
// `behind()` once the barrier behind the LAST operand read is passed.  !split (a block's last or only sub-window — no row to
// hold, and a lone matrix wave's operand work would only lengthen the phase —; a tuning build's bit 17: everywhere): eight Gram
// waves with one slice each, a SIMD's partner wave hides a wave's operand latency, nobody calls `behind()`.
// `full` (uniform in the block): the unmasked operand reads, see pipe_gram_mfma_lds.
// A sub-window of more than PIPE_GRAM_TILES_PER_ROUND tiles takes several rounds of the reduction buffer: the MFMAs of a round's
// tiles are issued in front of that round (a tile's accumulators — two sets on a matrix wave — live for one round only: the
// operands are read again from LDS, a tile's MFMAs are issued once).
// Barriers: every wave passes 2 * ceil(NT / TPR) - 1 of them, whatever its role: one per round, one between two rounds.
template <int QPL, int T, bool PACK, int R0, class Behind>
__device__ __forceinline__ void pipe_gram_round(const double *drows, int dstr, int W, int nvalid, const double *lw, double *gred,
                                                MCSAS_GLOBAL double *gout, MCSAS_GLOBAL double *scal_sub, bool split, bool full, bool matrix, Behind &&behind) {
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    constexpr int NT = PACK ? 2 : T * (T + 1) / 2;
    constexpr int TPR = PIPE_GRAM_TILES_PER_ROUND, RN = NT - R0 < TPR ? NT - R0 : TPR;
    if (matrix) {
        if (split) {
            if (full) pipe_gram_partials<QPL, T, PACK, R0, RN, 2, true>(drows, dstr, nvalid, lw, gred, wave);
            else pipe_gram_partials<QPL, T, PACK, R0, RN, 2, false>(drows, dstr, nvalid, lw, gred, wave);
        } else {
            if (full) pipe_gram_partials<QPL, T, PACK, R0, RN, 1, true>(drows, dstr, nvalid, lw, gred, wave);
            else pipe_gram_partials<QPL, T, PACK, R0, RN, 1, false>(drows, dstr, nvalid, lw, gred, wave);
        }
    }
    PIPE_LDS_BARRIER();
    if (R0 + TPR >= NT && !matrix) behind();                  // every operand read lies in front of this round's barrier
    {
        const int u = tid >> 8, idx = tid & 255;
        const int tsel = R0 + u;
        if (tsel < NT) {
            double sum = 0.;
#pragma unroll
            for (int v = 0; v < PIPE_WAVES; ++v) sum += gred[(size_t)(v * TPR + u) * 256 + idx];
            if constexpr (PACK) pipe_gram_store_pack(tsel, idx, sum, gout, scal_sub);
            else pipe_gram_store<T>(tsel, idx, sum, W, gout, scal_sub);
        }
    }
    if constexpr (R0 + TPR < NT) {
        PIPE_LDS_BARRIER();
        pipe_gram_round<QPL, T, PACK, R0 + TPR>(drows, dstr, W, nvalid, lw, gred, gout, scal_sub, split, full, matrix, behind);
    }
}

template <int QPL, int T, bool PACK, class Behind>
__device__ __forceinline__ void pipe_prod_gram_lds_t(const double *drows, int dstr, int W, int nvalid, const double *lw,
                                                     double *gred, MCSAS_GLOBAL double *gout, MCSAS_GLOBAL double *scal_sub,
                                                     bool split, Behind &&behind) {
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const bool matrix = !split || wave < PIPE_WAVES / 2;      // uniform in the wave
    // (the row groups of a sub-window of 8 rows reach past it — rows the LDS buffer does not hold —: masked whatever nvalid is)
    const bool full = nvalid == W && (PACK || W == 16 * T);   // uniform in the block
    pipe_gram_round<QPL, T, PACK, 0>(drows, dstr, W, nvalid, lw, gred, gout, scal_sub, split, full, matrix, behind);
}

// (a sub-window of T 16-row groups has at least 2 T - 1 rows per wave: the QPL whose row registers that exceeds never see it,
// pipe_geometry's pick_w — the same rule as the scan block's cases in chain_pipe.h)
template <int QPL, class Behind>
__device__ __forceinline__ void pipe_prod_gram_lds(const double *drows, int dstr, int W, int nvalid, const double *lw,
                                                   double *gred, MCSAS_GLOBAL double *gout, MCSAS_GLOBAL double *scal_sub,
                                                   bool split, Behind &&behind) {
    if (W == 24) { pipe_prod_gram_lds_t<QPL, 2, true>(drows, dstr, W, nvalid, lw, gred, gout, scal_sub, split, behind); return; }
    switch ((W + 15) >> 4) {                                   // uniform for the launch
#define PIPE_GRAM_CASE(T) case T: if constexpr ((2 * T - 1) * QPL <= PIPE_MAX_ROW_DOUBLES) pipe_prod_gram_lds_t<QPL, T, false>(drows, dstr, W, nvalid, lw, gred, gout, scal_sub, split, behind); break;
        PIPE_GRAM_CASE(1) PIPE_GRAM_CASE(2) PIPE_GRAM_CASE(3) PIPE_GRAM_CASE(4)
#undef PIPE_GRAM_CASE
        default: break;
    }
}

#ifdef MCSAS_TUNING
// ---- the Gram block in UNITS, for producers that evaluate the next sub-window's rows at the same time ----------------
// Rows without an integral: the Gram MFMAs of sub-window s are issued BETWEEN the rows of sub-window s + 1 (the matrix
// pipe runs beside the vector pipe: while one wave of a SIMD is inside a run of MFMAs its partner has the vector issue
// slots to itself), so a wave's share of a block — its q slice of 8 QPL points, every row — is cut into QPL units of 8 q
// (two MFMA k-steps per tile) that are done a few at a time.  Operands come from the window buffer the rows were just
// stored to (HBM/L2; same CU, same L1: visible to the whole workgroup once the storing waves have waited for their
// stores and passed a barrier).  The accumulators stay in registers between the calls.
// PACK (W = 24, three 8-row groups g0 g1 g2): the six upper-triangular 8x8 blocks fit TWO 16x16 tiles instead of the
// three of the 16-row grouping — tile 0 = rows [g0 g1] x columns [g1 g2] (blocks 01 02 11 12), tile 1 = rows and
// columns [g0 g2] (blocks 00 22; its 02 is a duplicate and not stored): a third fewer MFMAs.

template <int QPL, int T, bool PACK>
__device__ __forceinline__ void pipe_gram_units(const MCSAS_GLOBAL double *drows, int qpad, int nvalid, const double *lw, int gw,
                                                int u0, int u1, v4f64 (&acc)[PIPE_GRAM_NT_MAX]) {
    static_assert(T <= 2, "at most two 16-row groups per sub-window");
    const int lane = threadIdx.x & 63;
    const int m = lane & 15, kk = lane >> 4;
    constexpr int NL = PACK ? 3 : T;                          // row operands per lane and unit
    constexpr int SLICE = 64 * QPL / PIPE_WAVES;              // q per wave = 8 * (units per wave)
    static_assert(SLICE >= 8, "too many waves for this q count");
    const int qs = gw * SLICE + kk * 2;
    if (u0 == 0) {
#pragma unroll
        for (int i = 0; i < PIPE_GRAM_NT_MAX; ++i) acc[i] = (v4f64){0., 0., 0., 0.};
    }
    const MCSAS_GLOBAL double *rowp[NL];
    bool rowok[NL];
#pragma unroll
    for (int gi = 0; gi < NL; ++gi) {
        const int rr = PACK ? (gi == 0 ? m : gi == 1 ? 8 + m : (m < 8 ? m : m + 8)) : 16 * gi + m;
        rowok[gi] = rr < nvalid;
        rowp[gi] = drows + (size_t)(rowok[gi] ? rr : 0) * qpad + qs;
    }
    v2f64 cur[NL], nxt[NL];
#pragma unroll
    for (int gi = 0; gi < NL; ++gi) cur[gi] = *(const MCSAS_GLOBAL v2f64 *)(rowp[gi] + 8 * u0);
    for (int u = u0; u < u1; ++u) {
        const int un = u + 1 < u1 ? u + 1 : u;                // (the last unit is requested twice: no load under a condition)
#pragma unroll
        for (int gi = 0; gi < NL; ++gi) nxt[gi] = *(const MCSAS_GLOBAL v2f64 *)(rowp[gi] + 8 * un);
        const v2f64 wv = *reinterpret_cast<const v2f64 *>(lw + qs + 8 * u);
        v2f64 av[NL], bv[NL];
#pragma unroll
        for (int gi = 0; gi < NL; ++gi) {
            av[gi] = rowok[gi] ? cur[gi] : (v2f64){0., 0.};
            bv[gi] = av[gi] * wv;
        }
        if constexpr (PACK) {
            acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[0].x, bv[1].x, acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[2].x, bv[2].x, acc[1], 0, 0, 0);
            acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[0].y, bv[1].y, acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[2].y, bv[2].y, acc[1], 0, 0, 0);
        } else {
            int ti = 0;
#pragma unroll
            for (int gi = 0; gi < T; ++gi)
#pragma unroll
                for (int gj = gi; gj < T; ++gj) { acc[ti] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[gi].x, bv[gj].x, acc[ti], 0, 0, 0); ++ti; }
            ti = 0;
#pragma unroll
            for (int gi = 0; gi < T; ++gi)
#pragma unroll
                for (int gj = gi; gj < T; ++gj) { acc[ti] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[gi].y, bv[gj].y, acc[ti], 0, 0, 0); ++ti; }
        }
#pragma unroll
        for (int gi = 0; gi < NL; ++gi) cur[gi] = nxt[gi];
    }
}

// The same units with the operand loads and the MFMAs as two calls, so that a row evaluation fits between them: the loads
// of up to UCAP = 12 / NL units are in flight while the row is computed, the MFMAs run on landed operands.
constexpr int PIPE_GRAM_PREF = 12;                             // 16-byte operand registers per lane held across a row evaluation
template <int T, bool PACK> struct PipeGramScheme {
    static constexpr int NL = PACK ? 3 : T;
    static constexpr int UCAP = PIPE_GRAM_PREF / NL;
};
template <int QPL, int T, bool PACK>
__device__ __forceinline__ void pipe_gram_fetch(const MCSAS_GLOBAL double *drows, int qpad, int nvalid, int gw, int u0, int n,
                                                v2f64 (&G)[PIPE_GRAM_PREF]) {
    const int lane = threadIdx.x & 63;
    const int m = lane & 15, kk = lane >> 4;
    constexpr int NL = PipeGramScheme<T, PACK>::NL, UCAP = PipeGramScheme<T, PACK>::UCAP;
    constexpr int SLICE = 64 * QPL / PIPE_WAVES;
    const int qs = gw * SLICE + kk * 2;
#pragma unroll
    for (int gi = 0; gi < NL; ++gi) {
        const int rr = PACK ? (gi == 0 ? m : gi == 1 ? 8 + m : (m < 8 ? m : m + 8)) : 16 * gi + m;
        const MCSAS_GLOBAL double *rowp = drows + (size_t)(rr < nvalid ? rr : 0) * qpad + qs;
#pragma unroll
        for (int i = 0; i < UCAP; ++i) {
            const int u = u0 + (i < n ? i : n - 1);           // (past the chunk: its last unit again — no load under a condition)
            G[i * NL + gi] = *(const MCSAS_GLOBAL v2f64 *)(rowp + 8 * u);
        }
    }
}
template <int QPL, int T, bool PACK>
__device__ __forceinline__ void pipe_gram_consume(const v2f64 (&G)[PIPE_GRAM_PREF], int nvalid, const double *lw, int gw, int u0, int n,
                                                  v4f64 (&acc)[PIPE_GRAM_NT_MAX]) {
    const int lane = threadIdx.x & 63;
    const int m = lane & 15, kk = lane >> 4;
    constexpr int NL = PipeGramScheme<T, PACK>::NL, UCAP = PipeGramScheme<T, PACK>::UCAP;
    constexpr int SLICE = 64 * QPL / PIPE_WAVES;
    const int qs = gw * SLICE + kk * 2;
    if (u0 == 0) {
#pragma unroll
        for (int i = 0; i < PIPE_GRAM_NT_MAX; ++i) acc[i] = (v4f64){0., 0., 0., 0.};
    }
    bool rowok[NL];
#pragma unroll
    for (int gi = 0; gi < NL; ++gi) {
        const int rr = PACK ? (gi == 0 ? m : gi == 1 ? 8 + m : (m < 8 ? m : m + 8)) : 16 * gi + m;
        rowok[gi] = rr < nvalid;
    }
#pragma unroll
    for (int i = 0; i < UCAP; ++i)
        if (i < n) {                                          // uniform
            const v2f64 wv = *reinterpret_cast<const v2f64 *>(lw + qs + 8 * (u0 + i));
            v2f64 av[NL], bv[NL];
#pragma unroll
            for (int gi = 0; gi < NL; ++gi) {
                av[gi] = rowok[gi] ? G[i * NL + gi] : (v2f64){0., 0.};
                bv[gi] = av[gi] * wv;
            }
            if constexpr (PACK) {
                acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[0].x, bv[1].x, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[2].x, bv[2].x, acc[1], 0, 0, 0);
                acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[0].y, bv[1].y, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[2].y, bv[2].y, acc[1], 0, 0, 0);
            } else {
                int ti = 0;
#pragma unroll
                for (int gi = 0; gi < T; ++gi)
#pragma unroll
                    for (int gj = gi; gj < T; ++gj) { acc[ti] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[gi].x, bv[gj].x, acc[ti], 0, 0, 0); ++ti; }
                ti = 0;
#pragma unroll
                for (int gi = 0; gi < T; ++gi)
#pragma unroll
                    for (int gj = gi; gj < T; ++gj) { acc[ti] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[gi].y, bv[gj].y, acc[ti], 0, 0, 0); ++ti; }
            }
        }
}

// tiles per sub-window of the launch-uniform tile scheme (W <= 32 by pipe_geometry for these rows)
__device__ __forceinline__ int pipe_gram_tiles(int W) { return W == 24 ? 2 : (W <= 16 ? 1 : 3); }

// a wave's partial tiles -> its slots of the reduction buffer gred[wave][tile][256]
__device__ __forceinline__ void pipe_gram_park(const v4f64 (&acc)[PIPE_GRAM_NT_MAX], int nt, double *gred, int wave, int lane) {
#pragma unroll
    for (int ti = 0; ti < PIPE_GRAM_NT_MAX; ++ti)
        if (ti < nt) {
#pragma unroll
            for (int r = 0; r < 4; ++r) gred[((size_t)(wave * PIPE_GRAM_NT_MAX + ti) * 4 + r) * 64 + lane] = acc[ti][r];
        }
}

// all threads: the eight waves' partial tiles summed in wave order (deterministic), Gram block to gout[a][k] (a, k < W), and
// its diagonal — g_k = sum_q w d_k^2, the third of a step's ft-independent sums — to scal_sub[k][2]
__device__ __forceinline__ void pipe_gram_sum_store(int W, const double *gred, MCSAS_GLOBAL double *gout, MCSAS_GLOBAL double *scal_sub) {
    const int tid = threadIdx.x;
    const int nt = pipe_gram_tiles(W);
    for (int e = tid; e < nt * 256; e += PIPE_BLOCK) {
        const int ti = e >> 8, idx = e & 255;
        double sum = 0.;
#pragma unroll
        for (int v = 0; v < PIPE_WAVES; ++v) sum += gred[(size_t)(v * PIPE_GRAM_NT_MAX + ti) * 256 + idx];
        const int i = 4 * (idx >> 6) + ((idx & 63) >> 4), j = idx & 15;   // result register r of lane l holds D[4 r + l / 16][l % 16]
        int ar = -1, kc = -1;
        if (W == 24) {
            if (ti == 0) { ar = i; kc = 8 + j; }
            else if ((i < 8) == (j < 8)) { ar = i < 8 ? i : i + 8; kc = j < 8 ? j : j + 8; }
        } else {
            const int tgi = ti == 2 ? 1 : 0, tgj = ti == 0 ? 0 : 1;     // tiles (0,0), (0,1), (1,1)
            ar = 16 * tgi + i; kc = 16 * tgj + j;
        }
        if (ar >= 0 && ar < W && kc < W) {
            gout[(size_t)ar * W + kc] = sum;
            if (ar == kc) scal_sub[ar * 4 + 2] = sum;
        }
    }
}
#endif  // MCSAS_TUNING

}  // namespace mcsas
