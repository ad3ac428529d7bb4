// host_result.h — the one writer of a mcsas_result (include/mcsas_hip.h).  Every array of a result ends in the repetition:
// contribs[n_contrib][n_active][R], fit[nq][R] and the scalar arrays of the list below, [R] each; an array the caller left NULL is
// not written.  The entry points hold what they write in other shapes — a fetch the chains' records and [rep][...] blocks, the
// device-list path finished results of its blocks — and all of them place it through this file, at a repetition offset where the
// block is part of a longer result.  Plain host C++ without HIP: tests/result_writer_check.cpp compiles it alone, under sanitizers.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/mcsas_hip.h"

#pragma GCC visibility push(hidden)

// the per-repetition scalars of a result: X(field, element type).  ChainOut (chain_common.h) has a member of each name.
#define MCSAS_RESULT_SCALARS(X) \
    X(chisq, double) X(scaling, double) X(background, double) X(num_iter, int64_t) X(num_moves, int64_t) \
    X(attempts, int32_t) X(converged, int32_t) X(seconds, double) X(draws, int64_t)

// one repetition's scalars, for a source that keeps them under other names
struct ResultRow {
#define X(f, T) T f;
    MCSAS_RESULT_SCALARS(X)
#undef X
};

// repetition r of every scalar array, from anything with a member per field (ChainOut, ResultRow)
template <class Src> inline void result_put_row(mcsas_result *res, size_t r, const Src &src) {
#define X(f, T) if (res->f) res->f[r] = (T)src.f;
    MCSAS_RESULT_SCALARS(X)
#undef X
}

// columns [f0, f0 + Rg) of dst[rows][R] from a block whose element (i, r) lies at src[i * si + r * sr]; a NULL dst is skipped
template <class T> inline void result_put_block(T *dst, size_t rows, size_t R, size_t f0, size_t Rg, const T *src, size_t si, size_t sr) {
    if (!dst) return;
    for (size_t r = 0; r < Rg; ++r)
        for (size_t i = 0; i < rows; ++i) dst[i * R + f0 + r] = src[i * si + r * sr];
}
// Rg repetitions' parameter sets [rep][N][P] into contribs[(n * P + p) * R + f0 + rep] ...
inline void result_put_sets(mcsas_result *res, const double *sets, size_t N, size_t P, size_t R, size_t f0, size_t Rg) {
    result_put_block(res->contribs, N * P, R, f0, Rg, sets, 1, N * P);
}
// ... and their fits [rep][qpad], of which Q values count, into fit[k * R + f0 + rep]
inline void result_put_fit(mcsas_result *res, const double *fit, size_t qpad, size_t Q, size_t R, size_t f0, size_t Rg) {
    result_put_block(res->fit, Q, R, f0, Rg, fit, 1, qpad);
}

// A result of Rg repetitions with memory of its own: the arrays that `like` has, and no others.  put() places it as repetitions
// [f0, f0 + Rg) of a result of R (the blocks of a device list, mcsas_hip_analyse).
struct ResultPart {
    mcsas_result out{};                                       // (no array until make(): put() then writes nothing)
    std::vector<double> contribs, fit;
#define X(f, T) std::vector<T> f;
    MCSAS_RESULT_SCALARS(X)
#undef X
    void make(const mcsas_result *like, size_t NP, size_t Q, size_t Rg) {
        memset(&out, 0, sizeof out);
        out.struct_size = sizeof(mcsas_result);
        if (like->contribs) { contribs.resize(NP * Rg); out.contribs = contribs.data(); }
        if (like->fit) { fit.resize(Q * Rg); out.fit = fit.data(); }
#define X(f, T) if (like->f) { f.resize(Rg); out.f = f.data(); }
        MCSAS_RESULT_SCALARS(X)
#undef X
    }
    void put(mcsas_result *res, size_t NP, size_t Q, size_t R, size_t f0, size_t Rg) const {
        if (out.contribs) result_put_block(res->contribs, NP, R, f0, Rg, (const double *)out.contribs, Rg, 1);
        if (out.fit) result_put_block(res->fit, Q, R, f0, Rg, (const double *)out.fit, Rg, 1);
#define X(f, T) if (out.f) result_put_block(res->f, 1, R, f0, Rg, (const T *)out.f, Rg, 1);
        MCSAS_RESULT_SCALARS(X)
#undef X
    }
};

#pragma GCC visibility pop
