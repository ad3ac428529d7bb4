// result_writer_check.cpp — the one writer of a mcsas_result (mcsas_amd/csrc/host_result.h) on synthetic records, as a plain host
// program: tests/test_result_writer_host.py compiles it with -fsanitize=address,undefined and runs it.  R = 5 repetitions of N = 3
// contributions with P = 2 parameters, nq = 65 in rows of qpad = 128.  A result is filled whole, as blocks of 2 + 2 + 1 repetitions
// at their offsets and as the blocks of a list of 7 (two of them empty), each from [rep][...] records and through ResultPart (the
// device-list path); the fillings must be equal, every second array of the result is NULL (both parities), and every array lies
// between guard words.  Exit status 0 and "ok" when all of it holds.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../mcsas_amd/csrc/host_result.h"

static const size_t R = 5, N = 3, P = 2, Q = 65, QPAD = 128;
static const double GUARD = -12345.0, UNTOUCHED = -1.0, PADDING = -777.0;

template <class T> struct Guarded {                       // [guard | n values | guard], exactly: a write beside it is a heap overflow
    std::vector<T> v;
    Guarded(size_t n, bool null) { if (!null) { v.assign(n + 2, (T)UNTOUCHED); v.front() = v.back() = (T)GUARD; } }
    T *data() { return v.empty() ? nullptr : v.data() + 1; }
    bool guards_ok() const { return v.empty() || (v.front() == (T)GUARD && v.back() == (T)GUARD); }
};

// the arrays of a result; those whose index in the list (contribs 0, fit 1, then the scalars) has parity `null_parity` are NULL
struct Out {
    Guarded<double> contribs, fit;
#define X(f, T) Guarded<T> f;
    MCSAS_RESULT_SCALARS(X)
#undef X
    mcsas_result res{};
    static bool null_at(int &i, int parity) { return (i++ & 1) == parity; }
    explicit Out(int parity, int i = 0)
        : contribs(N * P * R, null_at(i, parity)), fit(Q * R, null_at(i, parity))
#define X(f, T) , f(R, null_at(i, parity))
          MCSAS_RESULT_SCALARS(X)
#undef X
    {
        res.struct_size = sizeof res;
        res.contribs = contribs.data(); res.fit = fit.data();
#define X(f, T) res.f = f.data();
        MCSAS_RESULT_SCALARS(X)
#undef X
    }
    bool guards_ok() const {
        bool ok = contribs.guards_ok() && fit.guards_ok();
#define X(f, T) ok = ok && f.guards_ok();
        MCSAS_RESULT_SCALARS(X)
#undef X
        return ok;
    }
    bool operator==(const Out &o) const {
        bool eq = contribs.v == o.contribs.v && fit.v == o.fit.v;
#define X(f, T) eq = eq && f.v == o.f.v;
        MCSAS_RESULT_SCALARS(X)
#undef X
        return eq;
    }
};

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { ++failures; fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); } } while (0)

// repetitions [first, first + count) of the G blocks (the split of mcsas_hip_shard)
static void block(size_t G, size_t g, size_t *first, size_t *count) {
    const size_t base = R / G, extra = R % G;
    *count = base + (g < extra ? 1 : 0);
    *first = g * base + (g < extra ? g : extra);
}

int main() {
    // the records: exact-size heap blocks, so that a read beside them is reported too
    std::vector<double> sets(R * N * P), fits(R * QPAD, PADDING);
    std::vector<ResultRow> rows(R);
    for (size_t r = 0; r < R; ++r) {
        for (size_t n = 0; n < N; ++n) for (size_t p = 0; p < P; ++p) sets[(r * N + n) * P + p] = 1000.0 * r + 10.0 * n + p + 0.5;
        for (size_t k = 0; k < Q; ++k) fits[r * QPAD + k] = 100.0 * r + k + 0.25;
        rows[r] = ResultRow{1.5 + r, 2.5 + r, 3.5 + r, (int64_t)(40 + r), (int64_t)(50 + r), (int32_t)(6 + r), (int32_t)(r & 1), 7.5 + r, ((int64_t)1 << 40) + (int64_t)r};
    }
    auto put_records = [&](mcsas_result *res, size_t total, size_t f0, size_t first, size_t count) {   // records [first, first + count) as repetitions f0... of `total`
        result_put_sets(res, sets.data() + first * N * P, N, P, total, f0, count);
        result_put_fit(res, fits.data() + first * QPAD, QPAD, Q, total, f0, count);
        for (size_t r = 0; r < count; ++r) result_put_row(res, f0 + r, rows[first + r]);
    };
    for (int parity = 0; parity < 2; ++parity) {
        Out whole(parity);
        put_records(&whole.res, R, 0, 0, R);
        CHECK(whole.guards_ok());
        for (size_t r = 0; r < R; ++r) {                  // the layout itself: the repetition is the last index
            if (whole.res.contribs) for (size_t i = 0; i < N * P; ++i) CHECK(whole.res.contribs[i * R + r] == sets[r * N * P + i]);
            if (whole.res.fit) for (size_t k = 0; k < Q; ++k) CHECK(whole.res.fit[k * R + r] == fits[r * QPAD + k]);
#define X(f, T) if (whole.res.f) CHECK(whole.res.f[r] == rows[r].f);
            MCSAS_RESULT_SCALARS(X)
#undef X
        }
        CHECK((whole.res.contribs == nullptr) != (whole.res.fit == nullptr));
        for (size_t G : {(size_t)3, (size_t)7}) {
            Out direct(parity), parts(parity);
            size_t seen = 0, empty = 0;
            for (size_t g = 0; g < G; ++g) {
                size_t first, count;
                block(G, g, &first, &count);
                seen += count; empty += count == 0;
                put_records(&direct.res, R, first, first, count);
                ResultPart part;                           // a block's own result of `count` repetitions, then at its place
                if (count) { part.make(&parts.res, N * P, Q, count); put_records(&part.out, count, 0, first, count); }
                part.put(&parts.res, N * P, Q, R, first, count);
            }
            CHECK(seen == R && empty == (G == 7 ? 2u : 0u));
            CHECK(direct.guards_ok() && parts.guards_ok());
            CHECK(direct == whole);
            CHECK(parts == whole);
        }
    }
    if (failures) return 1;
    printf("ok\n");
    return 0;
}
