// host_rows.hip — chains whose intensity rows the CALLER evaluates: on the host (mcsas_hip_analyse_host_rows, ABI 4) or on the device
// into a buffer of its own (mcsas_hip_analyse_device_rows).  The one unit that compiles chain_feed.h's two kernels; it knows no plan.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <vector>

#include "host_decide.h"     // fill_chain_settings
#include "host_result.h"
#include "chain_feed.h"     // feed_rows_kernel, feed_draw_kernel

using namespace mcsas;

// ------------------------------------------------------------------------------ rows evaluated by the caller on the host
// Philox4x32-10 on the host: the stream of device_util.h's philox_uniform (counter = (idx >> 1, chain, 0), key = seed; even draws
// take words 0,1, odd draws words 2,3; 53 bits)
static double philox_uniform_host(uint64_t seed, uint32_t chain, uint64_t idx) {
    const uint64_t blk = idx >> 1;
    uint32_t c0 = (uint32_t)blk, c1 = (uint32_t)(blk >> 32), c2 = chain, c3 = 0u;
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    const uint32_t a = (idx & 1) ? c2 : c0, b = (idx & 1) ? c3 : c1;
    return ((double)(a >> 5) * 67108864.0 + (double)(b >> 6)) / 9007199254740992.0;
}

// what both entry points refuse of a problem, before a device is touched
static int check_rows_problem(const mcsas_problem *p) {
    if (p->struct_size != sizeof(mcsas_problem))
        return fail(MCSAS_EINVAL, "mcsas_problem size %u, library expects %zu (ABI mismatch)", p->struct_size, sizeof(mcsas_problem));
    if (p->nq < 1 || p->nq > Q_MAX_SPLIT || !p->q || !p->intensity || !p->sigma) return fail(MCSAS_EINVAL, "nq %d (1..%d) / data pointers", p->nq, Q_MAX_SPLIT);
    if (p->n_active < 1 || p->n_active > MCSAS_MAX_ACTIVE) return fail(MCSAS_EINVAL, "n_active %d (1..%d)", p->n_active, MCSAS_MAX_ACTIVE);
    if (p->n_contrib < 1 || p->n_reps < 1 || p->max_iter < 0 || p->max_retries < 0) return fail(MCSAS_EINVAL, "n_contrib / n_reps / max_iter / max_retries");
    if (p->reserved0) return fail(MCSAS_EINVAL, "reserved0 must be 0");
    for (int c = 0; c < p->n_active; ++c)
        if (p->gen_kind[c] < MCSAS_GEN_UNIFORM || p->gen_kind[c] > MCSAS_GEN_EXP3) return fail(MCSAS_EINVAL, "gen_kind[%d] = %d", c, p->gen_kind[c]);
    return MCSAS_OK;
}

// rows per round: every chain's block is at most max(N, window) rows; as many chains per round as fit ~256 MB of rows
static void rows_shape(const mcsas_problem *p, int32_t window, size_t *blk, size_t *round_rows, size_t *qpad) {
    *qpad = ((size_t)p->nq + 63) / 64 * 64;
    *blk = std::max((size_t)p->n_contrib, (size_t)(window < 1 ? 64 : window));
    *round_rows = std::max(*blk, std::min((size_t)p->n_reps * *blk, (size_t)(256u << 20) / (*qpad * sizeof(double))));
}

// The chains of one such call, between the rounds: their state on the device (what feed_rows_kernel works on) and where the host
// has each of them in its random stream and in the retry loop of McSAS.analyse (mcsas.py:220-246).  A round is plan_round (which
// chains get rows, and where), the caller's rows, upload_meta and decide.  The device is selected by then.
struct FeedRun {
    struct HostChain { uint64_t draw_pos = 0; int64_t num_iter = 0, total = 0; int attempt = 0, phase = 0 /*0 init due, 1 running, 2 done*/, converged = 0, stopped = 0; double seconds = 0; };
    const mcsas_problem *p;
    const size_t R, N, P, Q, qpad;
    const int64_t window;
    const std::chrono::steady_clock::time_point t_begin = std::chrono::steady_clock::now();
    FeedArgs fa;
    DevBuf<double> dw, dwI, dI, drset, dcache, dft, dfit;
    DevBuf<FeedState> dstate;
    DevBuf<int64_t> dmeta;
    std::vector<HostChain> hc;
    std::vector<FeedState> hs;
    // the round's metadata, one upload: [2R] int64 (where each chain's attempt starts in its stream, the steps it has taken: what
    // feed_draw_kernel reads), then [3R] int32 (first row, row count, FEED_* of each chain)
    std::vector<int64_t> meta;
    size_t done = 0;
    bool stop_seen = false;

    FeedRun(const mcsas_problem *p_, size_t qpad_, int32_t window_)
        : p(p_), R(p_->n_reps), N(p_->n_contrib), P(p_->n_active), Q(p_->nq), qpad(qpad_), window(window_), hc(R), hs(R), meta(2 * R + (3 * R + 1) / 2) {}
    int64_t *pos() { return meta.data(); }
    int32_t *rows_of() { return reinterpret_cast<int32_t *>(meta.data() + 2 * R); }

    // data vectors, their sums and the settings, as mcsas_hip_plan_create prepares them; the rows and parameter sets of a round at `rows`, `pvals`
    int setup(const double *rows, const double *pvals) {
        memset(&fa, 0, sizeof fa);
        ChainArgs &a = fa.c;
        const WeighedData h(p, qpad, &a);
        HIPCHK(dw.alloc(qpad)); HIPCHK(dwI.alloc(qpad)); HIPCHK(dI.alloc(qpad));
        HIPCHK(drset.alloc(R * N * P)); HIPCHK(dcache.alloc(R * N * qpad)); HIPCHK(dft.alloc(R * qpad)); HIPCHK(dfit.alloc(R * qpad));
        HIPCHK(dstate.alloc(R)); HIPCHK(dmeta.alloc(meta.size()));
        HIPCHK(hipMemcpy(dw.p, h.w.data(), sizeof(double) * qpad, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(dwI.p, h.wI.data(), sizeof(double) * qpad, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(dI.p, h.I.data(), sizeof(double) * qpad, hipMemcpyHostToDevice));
        HIPCHK(hipMemset(dstate.p, 0, sizeof(FeedState) * R));
        HIPCHK(hipMemset(dfit.p, 0, sizeof(double) * R * qpad));

        a.model.n_active = (int)P;
        a.w = dw.p; a.wI = dwI.p; a.I = dI.p;
        fill_chain_settings(p, &a);                                             // (feed_draw_kernel reads the generators, seed and rep_offset)
        a.rset = drset.p; a.cache = dcache.p; a.cache_rows = (int)N; a.fit = dfit.p;
        fa.ft = dft.p; fa.state = dstate.p; fa.rows = rows; fa.pvals = pvals;
        const int32_t *dm = reinterpret_cast<const int32_t *>(dmeta.p + 2 * R);
        fa.first = dm; fa.count = dm + R; fa.kind = dm + 2 * R;
        return MCSAS_OK;
    }

    // which chains get rows in the next round of at most `round_rows` rows; returns how many rows that is
    size_t plan_round(size_t round_rows) {
        if (p->stop && *p->stop) stop_seen = true;
        size_t nrows = 0;
        std::fill(meta.begin(), meta.end(), 0);
        int32_t *m = rows_of();
        for (size_t r = 0; r < R; ++r) {
            HostChain &h = hc[r];
            if (h.phase == 2) continue;
            if (stop_seen) {                                                    // McSAS.stop (mcsas.py:357): end every chain where it is
                if (h.phase == 1) { m[2 * R + r] = FEED_END; h.stopped = 1; }
                else { h.phase = 2; h.stopped = 1; ++done; }
                continue;
            }
            const size_t want = h.phase == 0 ? N : (size_t)std::min<int64_t>(window, p->max_iter - h.num_iter);
            if (nrows + want > round_rows) continue;                            // next round
            m[r] = (int32_t)nrows; m[R + r] = (int32_t)want; m[2 * R + r] = h.phase == 0 ? FEED_INIT : FEED_STEPS;
            pos()[r] = (int64_t)h.draw_pos; pos()[R + r] = h.num_iter;
            nrows += want;
        }
        return nrows;
    }
    int upload_meta() {
        HIPCHK(hipMemcpy(dmeta.p, meta.data(), sizeof(int64_t) * meta.size(), hipMemcpyHostToDevice));
        return MCSAS_OK;
    }
    // the decisions on the round's rows, and what they mean for the chains
    int decide() {
        hipLaunchKernelGGL(feed_rows_kernel, dim3((unsigned)R), dim3(64), 0, nullptr, fa);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpy(hs.data(), dstate.p, sizeof(FeedState) * R, hipMemcpyDeviceToHost));
        const double now = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count();
        const int32_t *m = rows_of();
        for (size_t r = 0; r < R; ++r) {
            HostChain &h = hc[r];
            const int kind = m[2 * R + r];
            if (h.phase == 2 || (m[R + r] == 0 && kind != FEED_END)) continue;
            if (kind == FEED_INIT) { h.phase = 1; h.num_iter = 0; if (!p->start_from_minimum) h.draw_pos += (uint64_t)N * P; }   // the host's MCSAS_INITIAL_DRAWS (chain_common.h)
            h.num_iter = hs[r].num_iter;
            if (hs[r].ended) {                                                  // the attempt is over (mcsas.py:424-439)
                h.total += h.num_iter; h.draw_pos += (uint64_t)h.num_iter * P;
                h.converged = hs[r].converged;
                if (h.converged || h.stopped || h.attempt >= p->max_retries) { h.phase = 2; h.seconds = now; ++done; }
                else { ++h.attempt; h.phase = 0; }                              // :220-246: the next attempt goes on in the stream
            }
        }
        return MCSAS_OK;
    }
    int results(mcsas_result *res);
};

static int host_rows_run(const mcsas_problem *p, mcsas_rows_callback rows_cb, void *user, int32_t window, mcsas_result *res) {
    DeviceGuard guard;
    { int rc = select_device(p->device); if (rc) return rc; }
    size_t blk, round_rows, qpad;
    rows_shape(p, window, &blk, &round_rows, &qpad);
    FeedRun run(p, qpad, window);
    const size_t R = run.R, N = run.N, P = run.P, Q = run.Q;
    DevBuf<double> drows, dpv;
    HIPCHK(drows.alloc(round_rows * qpad)); HIPCHK(dpv.alloc(round_rows * P));
    if (int rc = run.setup(drows.p, dpv.p)) return rc;
    std::vector<double> pset(round_rows * P), hrows(round_rows * Q), staged(round_rows * qpad, 0.);
    // (a window is drawn ahead of the decisions: a draw behind the replay stream's end is no error here — the chain may end before
    // the step that would need it; what was consumed is known when the chain is through, see below)
    auto uniform = [&](size_t r, uint64_t idx) -> double {
        if (p->replay_stream) {
            if ((int64_t)idx < p->replay_len) return p->replay_stream[r * (size_t)p->replay_len + idx];
            return 0.5;
        }
        return philox_uniform_host(p->seed, (uint32_t)(p->rep_offset + (int)r), idx);
    };
    auto generate = [&](int c, double u) -> double {                      // numbergenerator.py:28-31,168-191; parameter.py:66-84
        if (p->gen_kind[c] != MCSAS_GEN_UNIFORM) {
            const double up = (double)p->gen_kind[c];
            u = (std::pow(10.0, 0.0 + (up - 0.0) * u) - 1.0) / (p->gen_kind[c] == 1 ? 10.0 : (p->gen_kind[c] == 2 ? 100.0 : 1000.0));
        }
        return u * (p->gen_hi[c] - p->gen_lo[c]) + p->gen_lo[c];
    };
    while (run.done < R) {
        const size_t nrows = run.plan_round(round_rows);
        const int32_t *first = run.rows_of(), *count = first + R, *kind = first + 2 * R;
        for (size_t r = 0; r < R; ++r) {
            const uint64_t draw_pos = (uint64_t)run.pos()[r];
            const int64_t num_iter = run.pos()[R + r];
            // host code for what the kernels take from chain_common.h ("how a chain draws": MCSAS_INITIAL_ROW, MCSAS_PROPOSAL_ROW,
            // draw_value as `generate`) and feed_draw_kernel restates for the device (chain_feed.h)
            for (size_t k = 0; k < (size_t)count[r]; ++k)
                for (size_t c = 0; c < P; ++c) {
                    double v;
                    if (kind[r] == FEED_INIT) v = p->start_from_minimum ? p->start_value[c]     // mcsas.py:310-317: N draws per parameter, parameter-major
                                                                        : generate((int)c, uniform(r, draw_pos + c * N + k));
                    else v = generate((int)c, uniform(r, draw_pos + (uint64_t)(num_iter + (int64_t)k) * P + c));   // :358
                    pset[((size_t)first[r] + k) * P + c] = v;
                }
        }
        if (nrows) {
            // ScatteringModel.calc's loop body for every row (scatteringmodel.py:90-99): the caller's calcIntensity
            const int rc = rows_cb(user, (int32_t)nrows, pset.data(), hrows.data());
            if (rc) return fail(MCSAS_ECALLBACK, "rows callback returned %d", rc);
            for (size_t i = 0; i < nrows; ++i) memcpy(&staged[i * qpad], &hrows[i * Q], sizeof(double) * Q);
            HIPCHK(hipMemcpy(drows.p, staged.data(), sizeof(double) * nrows * qpad, hipMemcpyHostToDevice));
            HIPCHK(hipMemcpy(dpv.p, pset.data(), sizeof(double) * nrows * P, hipMemcpyHostToDevice));
        }
        if (int rc = run.upload_meta()) return rc;
        if (int rc = run.decide()) return rc;
    }
    return run.results(res);
}

extern "C" int mcsas_hip_analyse_host_rows(const mcsas_problem *p, mcsas_rows_callback rows_cb, void *user, int32_t window,
                                           mcsas_result *res) {
    if (!p || !rows_cb || !res) return fail(MCSAS_EINVAL, "null argument");
    if (int rc = check_rows_problem(p)) return rc;
    return no_bad_alloc("analyse_host_rows", [&] { return host_rows_run(p, rows_cb, user, window < 1 ? 64 : window, res); });
}

// results in the layout of mcsas_result (mcsas.py:203-210,233-251)
int FeedRun::results(mcsas_result *res) {
    std::vector<double> hr(R * N * P), hf(R * qpad);
    HIPCHK(hipMemcpy(hr.data(), drset.p, sizeof(double) * hr.size(), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(hf.data(), dfit.p, sizeof(double) * hf.size(), hipMemcpyDeviceToHost));
    result_put_sets(res, hr.data(), N, P, R, 0, R);
    result_put_fit(res, hf.data(), qpad, Q, R, 0, R);
    int ovf = 0;
    for (size_t r = 0; r < R; ++r) {
        result_put_row(res, r, ResultRow{hs[r].chi2, hs[r].A, hs[r].b, hs[r].num_iter, hs[r].num_moves, hc[r].attempt + 1, hc[r].converged,
                                         hc[r].seconds, (int64_t)hc[r].draw_pos});
        // exhausted: a step the chain TOOK needed a draw behind the end — draw_pos counts the initial sets of the attempts that
        // were made and the steps that were decided, not what was drawn ahead for a window the chain left early
        if (p->replay_stream && (int64_t)hc[r].draw_pos > p->replay_len) ovf = 1;
    }
    if (ovf) return fail(MCSAS_ESTREAM, "replay stream exhausted (replay_len=%lld)", (long long)p->replay_len);
    return MCSAS_OK;
}

// ------------------------------------------------------------------------------ rows produced on the device by the caller
// The same rounds with nothing of them on the host: feed_draw_kernel writes the round's parameter sets into the caller's d_pset,
// the caller's device code fills d_rows, feed_rows_kernel decides on them where they lie.  Per round the metadata goes up and the
// chains' FeedState comes down; a replay stream is uploaded once.
// Measured once (one MI355X, 2026-10-19, tools/device_rows_ab.py -> profiles/device_rows_ab.md): a Sphere typed as a Python model,
// 100 q x 200 contributions x 10 repetitions x 20 000 steps, window 64 — 8.81 us of wall time per step through
// mcsas_hip_analyse_host_rows with a numpy model, 0.438 us through this entry point with the same model in torch: 20 times faster,
// the same accepted moves.  The device run is bound by its 314 rounds of launches and synchronisations (0.28 ms each), not by arithmetic.
extern "C" int mcsas_hip_device_rows_shape(const mcsas_problem *p, int32_t window, int64_t *min_rows, int64_t *useful_rows,
                                           int32_t *row_stride) {
    if (!p) return fail(MCSAS_EINVAL, "device_rows_shape: null problem");
    if (p->struct_size != sizeof(mcsas_problem))
        return fail(MCSAS_EINVAL, "mcsas_problem size %u, library expects %zu (ABI mismatch)", p->struct_size, sizeof(mcsas_problem));
    if (p->nq < 1 || p->nq > Q_MAX_SPLIT) return fail(MCSAS_EINVAL, "nq %d (1..%d)", p->nq, Q_MAX_SPLIT);
    if (p->n_contrib < 1 || p->n_reps < 1) return fail(MCSAS_EINVAL, "n_contrib / n_reps");
    size_t blk, round_rows, qpad;
    rows_shape(p, window, &blk, &round_rows, &qpad);
    if (min_rows) *min_rows = (int64_t)blk;
    if (useful_rows) *useful_rows = (int64_t)round_rows;
    if (row_stride) *row_stride = (int32_t)qpad;
    return MCSAS_OK;
}

// a buffer of the caller's must be device memory of the selected device before a kernel is launched on it (host_internal.h)
int check_device_buffer(const char *who, const char *name, const void *ptr, int dev) {
    hipPointerAttribute_t at;
    memset(&at, 0, sizeof at);
    const hipError_t e = hipPointerGetAttributes(&at, ptr);
    if (e != hipSuccess) {
        (void)hipGetLastError();                                               // (an unknown pointer is the caller's mistake, not a state to keep)
        return fail(MCSAS_EINVAL, "%s: %s is not device memory (%s)", who, name, hipGetErrorString(e));
    }
    if (at.type != hipMemoryTypeDevice || at.isManaged)
        return fail(MCSAS_EINVAL, "%s: %s is not device memory (memory type %d)", who, name, (int)at.type);
    if (at.device != dev) return fail(MCSAS_EINVAL, "%s: %s lies on device %d, the call runs on device %d", who, name, at.device, dev);
    return MCSAS_OK;
}

static int device_rows_run(const mcsas_problem *p, double *d_pset, double *d_rows, size_t round_rows, size_t capacity, size_t qpad,
                           mcsas_device_rows_callback rows_cb, void *user, int32_t window, mcsas_result *res) {
    DeviceGuard guard;
    { int rc = select_device(p->device); if (rc) return rc; }
    int dev = 0;
    HIPCHK(hipGetDevice(&dev));
    if (int rc = check_device_buffer("analyse_device_rows", "d_pset", d_pset, dev)) return rc;
    if (int rc = check_device_buffer("analyse_device_rows", "d_rows", d_rows, dev)) return rc;
    FeedRun run(p, qpad, window);
    if (int rc = run.setup(d_rows, d_pset)) return rc;
    ChainArgs &a = run.fa.c;
    DevBuf<double> dreplay;
    if (p->replay_stream) {
        const size_t len = (size_t)std::max<int64_t>(p->replay_len, 0);
        HIPCHK(dreplay.alloc(run.R * len));
        HIPCHK(hipMemcpy(dreplay.p, p->replay_stream, sizeof(double) * run.R * len, hipMemcpyHostToDevice));
        a.replay = dreplay.p; a.replay_len = (int64_t)len;
    }
    HIPCHK(hipMemset(d_rows, 0, sizeof(double) * capacity * qpad));            // the padding columns: the caller never writes them

    while (run.done < run.R) {
        const size_t nrows = run.plan_round(round_rows);
        if (int rc = run.upload_meta()) return rc;
        if (nrows) {
            hipLaunchKernelGGL(feed_draw_kernel, dim3((unsigned)run.R), dim3(64), 0, nullptr, run.fa, d_pset, (const int64_t *)run.dmeta.p);
            HIPCHK(hipGetLastError());
            HIPCHK(hipStreamSynchronize(nullptr));                             // the sets are complete before the caller reads them
            const int rc = rows_cb(user, (int32_t)nrows);
            if (rc) return fail(MCSAS_ECALLBACK, "rows callback returned %d", rc);
        }
        if (int rc = run.decide()) return rc;
    }
    return run.results(res);
}

extern "C" int mcsas_hip_analyse_device_rows(const mcsas_problem *p, double *d_pset, double *d_rows, int64_t capacity_rows,
                                             mcsas_device_rows_callback rows_cb, void *user, int32_t window, mcsas_result *res) {
    if (!p || !rows_cb || !res) return fail(MCSAS_EINVAL, "analyse_device_rows: null argument");
    if (!d_pset) return fail(MCSAS_EINVAL, "analyse_device_rows: d_pset is NULL");
    if (!d_rows) return fail(MCSAS_EINVAL, "analyse_device_rows: d_rows is NULL");
    if (int rc = check_rows_problem(p)) return rc;
    if (window < 1) window = 64;
    size_t blk, useful, qpad;
    rows_shape(p, window, &blk, &useful, &qpad);
    if (capacity_rows < (int64_t)blk)
        return fail(MCSAS_EINVAL, "analyse_device_rows: capacity_rows %lld < %lld = max(n_contrib, window), the rows of one chain's round (mcsas_hip_device_rows_shape)",
                    (long long)capacity_rows, (long long)blk);
    const size_t round_rows = std::min((size_t)capacity_rows, useful);
    return no_bad_alloc("analyse_device_rows", [&] { return device_rows_run(p, d_pset, d_rows, round_rows, (size_t)capacity_rows, qpad, rows_cb, user, window, res); });
}
