// host_analyse.hip — the one-shot entry points: an analysis, a batch of analyses, an analysis from a given start, a traced one, and
// an analysis spread over a device list.  Each makes plans, launches and fetches them through the public mcsas_hip_plan_* calls
// (mcsas_hip.hip) and destroys them; nothing in here sees inside a plan, and there is no kernel in this unit.
#include <hip/hip_runtime.h>

#include <string>
#include <thread>
#include <vector>

#include "host_internal.h"
#include "host_result.h"

using namespace mcsas;

// One-shot form: plans in the wavefront-per-chain mode for every problem, one batch launch, results at their places.
extern "C" int mcsas_hip_analyse_batch(const mcsas_problem *problems, int32_t n, mcsas_result *results) {
    if (!problems || !results || n < 1) return fail(MCSAS_EINVAL, "analyse_batch: needs n >= 1 problems and results (n = %d)", (int)n);
    for (int i = 0; i < n; ++i) {
        const mcsas_problem *p = &problems[i];
        if (p->struct_size != sizeof(mcsas_problem)) return fail(MCSAS_EINVAL, "analyse_batch: problem %d: mcsas_problem size %u, library expects %zu (ABI mismatch)", i, p->struct_size, sizeof(mcsas_problem));
        if (results[i].struct_size != sizeof(mcsas_result)) return fail(MCSAS_EINVAL, "analyse_batch: result %d: mcsas_result size mismatch", i);
        if (p->n_active == 0) continue;                                       // answered at its place below, as mcsas_hip_analyse does
        const WaveRequest wave = wave_request(p->exec_mode, p->nq);
        if (wave == WAVE_NOT_ASKED)
            return fail(MCSAS_EINVAL, "analyse_batch: problem %d asks for exec_mode %d; a batch runs one wavefront per chain (exec_mode 0 or 1)", i, p->exec_mode);
        if (p->n_devices > 1) return fail(MCSAS_EINVAL, "analyse_batch: problem %d spreads over %d devices; a batch runs on one", i, p->n_devices);
        if (wave == WAVE_TOO_MANY_Q) return fail(MCSAS_EINVAL, "analyse_batch: problem %d has nq %d > %d (one wavefront per chain)", i, p->nq, Q_MAX_WAVE);
    }
    std::vector<mcsas_plan *> plans;
    std::vector<int> index;
    int rc = MCSAS_OK;
    for (int i = 0; i < n && !rc; ++i) {
        if (problems[i].n_active == 0) continue;
        mcsas_problem p = problems[i];
        p.exec_mode = MCSAS_EXEC_WAVE;
        p.n_devices = 0;
        mcsas_plan *pl = nullptr;
        rc = mcsas_hip_plan_create(&p, &pl);
        if (rc) { std::string e = g_err; rc = fail(rc, "analyse_batch: problem %d: %s", i, e.c_str()); break; }
        plans.push_back(pl); index.push_back(i);
    }
    if (!rc && !plans.empty()) rc = mcsas_hip_plan_launch_batch(plans.data(), (int32_t)plans.size(), nullptr);
    if (!rc) {
        for (size_t k = 0; k < plans.size(); ++k) {
            const int rk = mcsas_hip_plan_fetch(plans[k], &results[index[k]]);
            if (rk && !rc) { std::string e = g_err; rc = fail(rk, "analyse_batch: problem %d: %s", index[k], e.c_str()); }
        }
    }
    for (mcsas_plan *pl : plans) mcsas_hip_plan_destroy(pl);
    if (rc) return rc;
    for (int i = 0; i < n; ++i)
        if (problems[i].n_active == 0) {
            const int r0 = mcsas_hip_analyse(&problems[i], &results[i]);
            if (r0) return r0;
        }
    return MCSAS_OK;
}

// `start` (or null): columns [rep_first, rep_first + n_reps) of start[n_contrib][n_active][rep_stride], mcsas_hip_plan_set_start
static int analyse_one(const mcsas_problem *p, mcsas_result *res, const double *start = nullptr, int32_t rep_stride = 0, int32_t rep_first = 0) {
    mcsas_plan *pl = nullptr;
    int rc = mcsas_hip_plan_create(p, &pl);
    if (rc) return rc;
    if (start) rc = mcsas_hip_plan_set_start(pl, start, rep_stride, rep_first);
    if (!rc) rc = mcsas_hip_plan_launch(pl, nullptr);
    if (!rc) rc = mcsas_hip_plan_fetch(pl, res);
    mcsas_hip_plan_destroy(pl);
    return rc;
}

// repetitions [first, first + count) of device-list entry `index` (contiguous blocks, sizes differ by at most one)
extern "C" int mcsas_hip_shard(int32_t n_reps, int32_t n_devices, int32_t index, int32_t *first, int32_t *count) {
    if (n_reps < 0 || n_devices < 1 || index < 0 || index >= n_devices || !first || !count) return fail(MCSAS_EINVAL, "bad argument");
    const int32_t base = n_reps / n_devices, extra = n_reps % n_devices;
    *count = base + (index < extra ? 1 : 0);
    *first = index * base + (index < extra ? index : extra);
    return MCSAS_OK;
}

// McSAS.analyse's repetition loop (mcsas.py:214-262) over several GPUs: one host thread, one plan and one stream per
// device, each running a contiguous block of repetitions under its global chain ids; every block lands in the caller's
// (…, numReps) arrays at its place.  No data-path exchange between the devices: the blocks share read-only inputs only.
static int analyse_sharded(const mcsas_problem *p, mcsas_result *res, const double *start = nullptr) {
    if (res->struct_size != sizeof(mcsas_result)) return fail(MCSAS_EINVAL, "mcsas_result size mismatch");
    const int G = p->n_devices;
    if (G > MCSAS_MAX_DEVICES) return fail(MCSAS_EINVAL, "n_devices %d > %d", G, MCSAS_MAX_DEVICES);
    if (p->n_reps < 1 || p->n_contrib < 1 || p->nq < 1) return fail(MCSAS_EINVAL, "n_reps, n_contrib and nq must be >= 1");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(MCSAS_ENODEV, "no HIP device available");
    for (int g = 0; g < G; ++g)
        if (p->devices[g] < 0 || p->devices[g] >= ndev) return fail(MCSAS_ENODEV, "devices[%d] = %d, %d present", g, p->devices[g], ndev);
    const size_t R = p->n_reps, N = p->n_contrib, P = p->n_active, Q = p->nq;
    struct Shard {
        mcsas_problem prob; ResultPart part;
        int32_t first = 0, count = 0; int rc = 0; std::string err;
    };
    std::vector<Shard> sh(G);
    std::vector<std::thread> th;
    for (int g = 0; g < G; ++g) {
        Shard &s = sh[g];
        mcsas_hip_shard((int32_t)R, G, g, &s.first, &s.count);
        if (s.count == 0) continue;
        s.prob = *p;
        s.prob.n_devices = 0; s.prob.device = p->devices[g];
        s.prob.n_reps = s.count; s.prob.rep_offset = p->rep_offset + s.first;
        if (p->replay_stream) s.prob.replay_stream = p->replay_stream + (size_t)s.first * p->replay_len;
        s.part.make(res, N * P, Q, (size_t)s.count);
        th.emplace_back([&s, start, R]() {
            s.rc = analyse_one(&s.prob, &s.part.out, start, (int32_t)R, s.first);   // (every block reads its own columns of the one start)
            if (s.rc) s.err = g_err;                          // (thread-local in the worker)
        });
    }
    for (auto &t : th) t.join();
    for (int g = 0; g < G; ++g)
        if (sh[g].rc) return fail(sh[g].rc, "device %d (repetitions %d..%d): %s", p->devices[g], sh[g].first, sh[g].first + sh[g].count - 1, sh[g].err.c_str());
    for (const Shard &s : sh)                                 // (a block without repetitions holds no array)
        s.part.put(res, N * P, Q, R, (size_t)s.first, (size_t)s.count);
    return MCSAS_OK;
}

extern "C" int mcsas_hip_analyse(const mcsas_problem *p, mcsas_result *res) {
    if (!res) return fail(MCSAS_EINVAL, "null result");
    if (p && p->n_active == 0) {
        // No active fit parameter (mcsas.py:198-201, 238-239, 322-323): analyse() runs ONE repetition of ONE
        // contribution, mcFit returns the model's intensity at its fixed parameter values with conval = -1,
        // scaling 1, background 0, and the repetition loop leaves without retrying.  Result arrays are sized
        // for n_contrib = n_reps = 1 whatever the problem says.
        if (res->struct_size != sizeof(mcsas_result)) return fail(MCSAS_EINVAL, "mcsas_result size mismatch");
        if (p->struct_size != sizeof(mcsas_problem)) return fail(MCSAS_EINVAL, "mcsas_problem size mismatch (ABI)");
        if (p->nq < 1 || !p->q) return fail(MCSAS_EINVAL, "nq/q missing");
        std::vector<double> cum(p->nq);
        int rc0 = mcsas_hip_model_calc(p, nullptr, 1, cum.data(), nullptr, nullptr, nullptr, nullptr);
        if (rc0) return rc0;
        result_put_fit(res, cum.data(), (size_t)p->nq, (size_t)p->nq, 1, 0, 1);
        result_put_row(res, 0, ResultRow{/*chisq*/ -1.0, /*scaling*/ 1.0, /*background*/ 0.0, /*num_iter*/ 0, /*num_moves*/ 0,
                                         /*attempts*/ 1, /*converged*/ 1, /*seconds*/ 0.0, /*draws*/ 0});
        return MCSAS_OK;
    }
    if (p && p->struct_size == sizeof(mcsas_problem) && p->n_devices > 1) return analyse_sharded(p, res);
    return analyse_one(p, res);
}

// What mcsas_hip_analyse_from (tr null: the start is the point of the call) and mcsas_hip_analyse_traced (tr: the caller's trace; a
// start may come with it) refuse, in the order they refuse it and before a device is touched, and the problem they run: *q, with the
// execution mode fixed to the kernel that takes a start and keeps a trace — one wavefront per chain, or, where MCSAS_EXEC_WORKGROUP
// is asked for more than 1024 q-points, the q-split kernel.  *fixed: no active parameter; nothing else was looked at, *q is not set.
static int start_or_trace_request(const char *who, const mcsas_problem *p, const double *start, const mcsas_result *res, const mcsas_trace *tr,
                                  bool traced, mcsas_problem *q, bool *fixed) {
    const char *const what = traced ? "trace" : "start";
    if (!p || !res) return fail(MCSAS_EINVAL, "%s: null argument", who);
    if (p->struct_size != sizeof(mcsas_problem))
        return fail(MCSAS_EINVAL, "%s: mcsas_problem size %u, library expects %zu (ABI mismatch)", who, p->struct_size, sizeof(mcsas_problem));
    if (traced) { if (int rc = check_trace_arrays(who, tr)) return rc; }
    *fixed = p->n_active == 0;
    if (*fixed) return MCSAS_OK;
    if (!traced && !start) return fail(MCSAS_EINVAL, "%s: start is NULL (mcsas_hip_analyse runs without one)", who);
    // (a start or a trace never picks the mode: MCSAS_EXEC_AUTO is one wavefront per chain here, the q-split kernel has to be asked for)
    const WaveRequest wave = wave_request(p->exec_mode, p->nq);
    const bool q_split = p->exec_mode == MCSAS_EXEC_WORKGROUP && runs_q_split(p->exec_mode, p->waves_per_chain, p->nq);
    if (wave == WAVE_NOT_ASKED && !q_split) {
        if (traced) return fail(MCSAS_EINVAL, "%s: exec_mode %d (%s) asked; a trace needs exec_mode = MCSAS_EXEC_WAVE (%d, or 0)", who, p->exec_mode, exec_mode_name(p->exec_mode), MCSAS_EXEC_WAVE);
        return fail(MCSAS_EINVAL, "%s: exec_mode %d (%s) asked with %d q-points; a start needs exec_mode = MCSAS_EXEC_WAVE (%d, or 0), or MCSAS_EXEC_WORKGROUP (%d) with more than %d q-points",
                    who, p->exec_mode, exec_mode_name(p->exec_mode), p->nq, MCSAS_EXEC_WAVE, MCSAS_EXEC_WORKGROUP, Q_MAX_WINDOW);
    }
    if (p->nq > Q_MAX_SPLIT) return fail(MCSAS_EINVAL, "%s: nq %d > %d is not supported", who, p->nq, Q_MAX_SPLIT);
    if (wave == WAVE_TOO_MANY_Q)
        return fail(MCSAS_EINVAL, "%s: nq %d > %d: one wavefront per chain does not take it, and with exec_mode %d a %s runs one wavefront per chain; "
                    "MCSAS_EXEC_WORKGROUP (%d) %s for %d...%d q-points", who, p->nq, Q_MAX_WAVE, p->exec_mode, what, MCSAS_EXEC_WORKGROUP,
                    traced ? "keeps a trace" : "takes a start", Q_MAX_WINDOW + 1, Q_MAX_SPLIT);
    if (traced && p->n_devices > 1) return fail(MCSAS_EINVAL, "%s: n_devices %d: a trace is kept on one device", who, p->n_devices);
    if (p->n_active < 0 || p->n_active > MCSAS_MAX_ACTIVE) return fail(MCSAS_EINVAL, "n_active %d out of range", p->n_active);
    if (p->n_contrib < 1 || p->n_reps < 1) return fail(MCSAS_EINVAL, "n_contrib and n_reps must be >= 1");
    if (traced && TraceLayout::too_large((size_t)p->n_reps, (size_t)tr->capacity, (size_t)p->n_active))
        return fail(MCSAS_EINVAL, "%s: %d repetitions x capacity %d x %d bytes per move exceed 2 GiB", who, p->n_reps, (int)tr->capacity, (int)TraceLayout(1, 0, (size_t)p->n_active).move_bytes);
    if (start) { if (int rc = check_start_finite(who, start, (size_t)p->n_contrib, (size_t)p->n_active, (size_t)p->n_reps, 0, (size_t)p->n_reps)) return rc; }
    *q = *p;
    q->exec_mode = q_split ? MCSAS_EXEC_WORKGROUP : MCSAS_EXEC_WAVE;
    return MCSAS_OK;
}

// McSAS.analyse with the first attempt of every repetition started from a given set (include/mcsas_hip.h)
extern "C" int mcsas_hip_analyse_from(const mcsas_problem *p, const double *start, mcsas_result *res) {
    mcsas_problem q;
    bool fixed = false;
    if (int rc = start_or_trace_request("analyse_from", p, start, res, nullptr, false, &q, &fixed)) return rc;
    if (fixed) return mcsas_hip_analyse(p, res);                               // nothing to start: one contribution at fixed values
    if (q.n_devices > 1) return analyse_sharded(&q, res, start);
    return analyse_one(&q, res, start, q.n_reps, 0);
}

// mcsas_hip_analyse (MCSAS_EXEC_WAVE), or mcsas_hip_analyse_from when a start is given, with the accepted moves of every repetition's
// last attempt (include/mcsas_hip.h)
extern "C" int mcsas_hip_analyse_traced(const mcsas_problem *p, const double *start, mcsas_result *res, mcsas_trace *tr) {
    mcsas_problem q;
    bool fixed = false;
    if (int rc = start_or_trace_request("analyse_traced", p, start, res, tr, true, &q, &fixed)) return rc;
    if (fixed) {                                                               // one contribution at fixed values: no move is ever made
        const int rc = mcsas_hip_analyse(p, res);
        if (!rc) tr->count[0] = 0;
        return rc;
    }
    q.n_devices = 0;
    mcsas_plan *pl = nullptr;
    int rc = mcsas_hip_plan_create(&q, &pl);
    if (rc) return rc;
    if (start) rc = mcsas_hip_plan_set_start(pl, start, q.n_reps, 0);
    if (!rc) rc = mcsas_hip_plan_set_trace(pl, tr->capacity);
    if (!rc) rc = mcsas_hip_plan_launch(pl, nullptr);
    if (!rc) rc = mcsas_hip_plan_fetch(pl, res);
    // (a replay stream that ran out is reported by the fetch; the trace of what ran is still the caller's)
    if (!rc || rc == MCSAS_ESTREAM) {
        const std::string e = g_err;
        const int rt = mcsas_hip_plan_fetch_trace(pl, 0, tr);
        if (rt) rc = rt; else g_err = e;
    }
    mcsas_hip_plan_destroy(pl);
    return rc;
}
