// host_decide.hip — what libmcsas_hip.so decides without a device: the refusals of a problem, a start and a trace, the execution mode
// and geometry of a problem (decide_shape), the settings block and the weights of every chain run, the request, layout and padded data
// of several sets fitted with one population, how a kernel family is launched and what a plug-in's instance of it is called, the
// transposition of a fetched trace block, the tick budget of a pipeline launch, and the error text every unit leaves.  No function
// in here calls the HIP runtime: tests/plan_decisions_check.hip links this file alone and runs on a machine without a GPU.  Like
// mcsas_hip.hip it tests MCSAS_TUNING (validate_problem, tune_word) and is built twice.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "host_decide.h"
#include "chain_wide.h" // WIDE_* constants only
#include "auto_table.h" // measured rates of the execution modes (tools/make_auto_table.py)
#include "model_list.h" // MCSAS_FOR_MODELS: the built-in models

using namespace mcsas;

// host_internal.h's q-point limits are the kernels': 16 q slots per lane, 64, and WIDE_MAX_WAVES waves of 32
static_assert(Q_MAX_WINDOW == 16 * WAVE && Q_MAX_WAVE == 64 * WAVE && Q_MAX_SPLIT == WIDE_MAX_WAVES * WAVE * 32, "host_internal.h: Q_MAX_*");

// ------------------------------------------------------------------------------ error plumbing
thread_local std::string g_err;
int fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    g_err = buf;
    return code;
}
int fail_within(int code, const char *fmt, ...) {
    const std::string why = g_err;
    char who[512];
    va_list ap; va_start(ap, fmt); vsnprintf(who, sizeof who, fmt, ap); va_end(ap);
    return fail(code, "%s: %s", who, why.c_str());
}

// ------------------------------------------------------------------------------ models and smearing: what a problem is refused for
ModelTraits model_traits(int model_id) {
#define TRAITS_OF(m) {Contrib<m>::INT_DIV_PARAM, Contrib<m>::ROWTAB, Contrib<m>::ROW_CLASS, Contrib<m>::CAN_SMEAR, &Contrib<m>::table_doubles, (int)(sizeof(Contrib<m>) / 8)},
    static const ModelTraits builtin[] = {MCSAS_FOR_MODELS(TRAITS_OF)};
#undef TRAITS_OF
    static_assert(sizeof builtin / sizeof builtin[0] == MCSAS_MODEL_COUNT, "model_list.h and include/mcsas_hip.h disagree");
    if (model_id >= 0 && model_id < MCSAS_MODEL_COUNT) return builtin[model_id];
    int row_class = 0;
    bool can_smear = false;
    (void)plugin_declares(model_id, &row_class, &can_smear);                          // plugin_model.h
    // (Contrib<MCSAS_MODEL_PLUGIN>, plugin_model.h: the full parameter vector and three doubles)
    return ModelTraits{-1, 0, row_class, can_smear, [](int) { return 0; }, MCSAS_MAX_PARAMS + 3};
}
static int model_int_div(const mcsas_problem *p) {
    const int i = model_traits(p->model_id).int_div_param;
    return i < 0 ? 1 : (int)p->params[i];
}

int fill_model_args(const mcsas_problem *p, ModelArgs *m) {
    if ((p->model_id < 0 || p->model_id >= MCSAS_MODEL_COUNT) && !(is_plugin_model(p->model_id) && plugin_declares(p->model_id, nullptr, nullptr)))
        return fail(MCSAS_EINVAL, "unknown model_id %d", p->model_id);
    if (p->n_active < 0 || p->n_active > MCSAS_MAX_ACTIVE) return fail(MCSAS_EINVAL, "n_active %d out of range", p->n_active);
    memset(m, 0, sizeof *m);
    m->model_id = p->model_id; m->n_active = p->n_active; m->comp_exp = p->comp_exp;
    for (int i = 0; i < MCSAS_MAX_PARAMS; ++i) m->params[i] = p->params[i];
    for (int c = 0; c < MCSAS_MAX_ACTIVE; ++c) {
        m->active_index[c] = c < p->n_active ? p->active_index[c] : -1;
        m->clip_lo[c] = p->clip_lo[c]; m->clip_hi[c] = p->clip_hi[c];
        if (c < p->n_active && (p->active_index[c] < 0 || p->active_index[c] >= MCSAS_MAX_PARAMS))
            return fail(MCSAS_EINVAL, "active_index[%d]=%d out of range", c, p->active_index[c]);
    }
    m->int_div = model_int_div(p);
    m->use_rowtab = rowtab_doubles_host(p->model_id, m->int_div) > 0;
    m->qmax = 0.;
    if (p->q) for (int i = 0; i < p->nq; ++i) m->qmax = std::max(m->qmax, std::fabs(p->q[i]));
    if (model_traits(p->model_id).int_div_param >= 0 && (m->int_div < 2 || m->int_div > 4096))
        return fail(MCSAS_EINVAL, "intDiv %d unsupported (2..4096)", m->int_div);
    return MCSAS_OK;
}

bool SmearDev::active(const mcsas_problem *p) { return p->smear_nk > 0 && model_traits(p->model_id).can_smear; }   // canSmear = False: not smeared
int SmearDev::check(const mcsas_problem *p) {
    const int K = p->smear_nk;
    if (active(p) && (K < 2 || K > 4096 || !p->smear_locs || !p->smear_q_offset || !p->smear_weights))
        return fail(MCSAS_EINVAL, "smearing: smear_nk %d (2..4096) needs locs, q_offset and weights", K);
    return MCSAS_OK;
}

// MCSAS_EXEC_AUTO, rows without an integral: nearest swept shape in (log q slots, log contributions), rates interpolated
// linearly in the repetition count, modes that cannot run the shape left out
static int auto_mode_light(int qpad, int n_contrib, double reps, bool pipe_ok, bool wg_ok) {
    if (reps < (double)auto_reps[0]) return pipe_ok ? MCSAS_EXEC_PIPELINE : (wg_ok ? MCSAS_EXEC_WORKGROUP : MCSAS_EXEC_WAVE);
    int iq = 0, in = 0;
    for (int i = 1; i < AUTO_NQ; ++i) if (std::fabs(std::log((double)qpad / auto_qpad[i])) < std::fabs(std::log((double)qpad / auto_qpad[iq]))) iq = i;
    for (int i = 1; i < AUTO_NN; ++i) if (std::fabs(std::log((double)n_contrib / auto_ncontrib[i])) < std::fabs(std::log((double)n_contrib / auto_ncontrib[in]))) in = i;
    int ir = 0;
    while (ir + 2 < AUTO_NR && reps >= (double)auto_reps[ir + 1]) ++ir;
    double f = (reps - auto_reps[ir]) / (double)(auto_reps[ir + 1] - auto_reps[ir]);
    f = f < 0. ? 0. : (f > 1. ? 1. : f);
    const float (&a)[3] = auto_rate[iq][in][ir], (&b)[3] = auto_rate[iq][in][ir + 1];
    const bool ok[3] = {true, wg_ok, pipe_ok};
    static const int modes[3] = {MCSAS_EXEC_WAVE, MCSAS_EXEC_WORKGROUP, MCSAS_EXEC_PIPELINE};
    int best = 0; double best_rate = -1.;
    for (int m = 0; m < 3; ++m) {
        if (!ok[m] || a[m] <= 0.f || b[m] <= 0.f) continue;
        const double r = a[m] + f * (b[m] - a[m]);
        if (r > best_rate) { best_rate = r; best = m; }
    }
    return modes[best];
}

// ------------------------------------------------------------------------------ how a problem runs
int validate_problem(const mcsas_problem *p) {
    if (p->struct_size != sizeof(mcsas_problem))
        return fail(MCSAS_EINVAL, "mcsas_problem size %u, library expects %zu (ABI mismatch)", p->struct_size, sizeof(mcsas_problem));
#ifndef MCSAS_TUNING
    if (p->reserved0 != 0) return fail(MCSAS_EINVAL, "mcsas_problem.reserved0 must be 0 (it is %d)", p->reserved0);
#endif
    if (p->nq < 1 || !p->q || !p->intensity || !p->sigma) return fail(MCSAS_EINVAL, "nq/q/intensity/sigma missing");
    if (p->n_contrib < 1 || p->n_reps < 1) return fail(MCSAS_EINVAL, "n_contrib and n_reps must be >= 1");
    if (p->n_active < 1) return fail(MCSAS_EINVAL, "a plan needs an active parameter (mcsas_hip_analyse answers the no-active-parameter case itself)");
    if (p->max_iter < 0 || p->max_retries < 0) return fail(MCSAS_EINVAL, "max_iter/max_retries negative");
    if (p->replay_stream && p->replay_len < 1) return fail(MCSAS_EINVAL, "replay_len must be >= 1");
    return MCSAS_OK;
}

TuneWord tune_word(const mcsas_problem *p) {
    TuneWord t;
#ifdef MCSAS_TUNING
    // measurement build (make tuning): mcsas_problem.reserved0 is the tuning / ablation word of the pipeline mode —
    // bits 8-11 rows per producer wave (0 = automatic), 12-15 cap on the scan sub-window in units of 8 steps, 16 every
    // proposal's `new` row stored and row slots swapped on acceptance (no lazy re-evaluation of stale rows), 17 all eight producer waves
    // on a sub-window's Gram MFMAs and no row beside them (pipe_gram.h: no matrix / row roles; read by the kernel), 18 the overlapped
    // producer (Gram MFMAs of sub-window s between the rows of s + 1, operands from HBM/L2), 19-20 row shares of a SIMD's two
    // producer waves, 21 matrix / row roles in EVERY sub-window's Gram phase, a block's last one included (pipe_prod.h; read by the kernel),
    // 7 XCD-aware block map; bits 0-6 switch stages OFF and give invalid results
    t.rpw = (p->reserved0 >> 8) & 15; t.sub = (p->reserved0 >> 12) & 15; t.gram_global = (p->reserved0 >> 18) & 1; t.eager = (p->reserved0 >> 16) & 1;
#else
    (void)p;
#endif
    return t;
}

int table_doubles_block(int model_id, int int_div, int waves_per_block) {
    return table_doubles_host(model_id, int_div) + waves_per_block * rowtab_doubles_host(model_id, int_div);
}

int decide_shape(const mcsas_problem *p, const ModelArgs &margs, int n_cus, size_t free_bytes, const TuneWord &tw, PlanShape *s) {
    *s = PlanShape{};
    // q slots per lane: power of two so the kernels are fully unrolled
    int qpl = 1;
    while (qpl * WAVE < p->nq && qpl < 64) qpl *= 2;
    // up to 1024 q-points every execution mode has kernels (q slots per lane 1..16).  More (un-binned data, nBin = 0):
    // one workgroup per chain with the q-points split over up to 8 waves (chain_wide.h; 8 / 16 / 32 slots per lane:
    // up to 4096 / 8192 / 16384 q-points) — MCSAS_EXEC_WORKGROUP, and what MCSAS_EXEC_AUTO picks; up to 4096 q-points
    // MCSAS_EXEC_WAVE still runs one wavefront per chain with 32 / 64 slots per lane
    const bool wide_q = p->nq > Q_MAX_WINDOW;
    const bool wide = runs_q_split(p->exec_mode, p->waves_per_chain, p->nq);
    int wide_waves = 0;
    if (wide_q) {
        if (p->exec_mode == MCSAS_EXEC_PIPELINE) return fail(MCSAS_EINVAL, "nq %d > %d: the pipeline has no kernels for it (exec_mode 0, 1 or 2)", p->nq, Q_MAX_WINDOW);
        if (p->nq > Q_MAX_SPLIT) return fail(MCSAS_EINVAL, "nq %d > %d is not supported", p->nq, Q_MAX_SPLIT);
        if (!wide && p->nq > Q_MAX_WAVE) return fail(MCSAS_EINVAL, "nq %d > %d runs one workgroup per chain only (exec_mode 0 or 2)", p->nq, Q_MAX_WAVE);
        if (wide) {
            for (qpl = 8; qpl * WAVE * WIDE_MAX_WAVES < p->nq;) qpl *= 2;               // 8 / 16 / 32 slots per lane
            wide_waves = (p->nq + qpl * WAVE - 1) / (qpl * WAVE);
        }
    }
    const int qpad = wide ? qpl * WAVE * wide_waves : qpl * WAVE;
    if (int rc = SmearDev::check(p)) return rc;
    // rows that cost a numerical integration each (2: and whose cost varies with the parameter set — pipe_layout.h, pipe_geometry)
    const int heavy_rows = std::max(model_traits(p->model_id).row_class, SmearDev::active(p) ? 1 : 0);
    const int contrib_doubles = model_traits(p->model_id).contrib_doubles;
    auto tabd = [&](int waves_per_block) { return table_doubles_block(p->model_id, margs.int_div, waves_per_block); };
    const int N = p->n_contrib;
    // execution mode (results do not depend on it)
    int mode = p->exec_mode;
    int waves = p->waves_per_chain;
    if (is_plugin_model(p->model_id) && wide_q && !wide)
        return fail(MCSAS_EINVAL, "model plug-ins: more than 1024 q-points run one workgroup per chain only (exec_mode 0 or 2; nq %d, exec_mode %d asked)", p->nq, p->exec_mode);
    if (mode == MCSAS_EXEC_AUTO) {
        if (waves == 1) mode = MCSAS_EXEC_WAVE;
        else if (waves > 1) mode = MCSAS_EXEC_WORKGROUP;
        else {
            PipeGeom pg; WgGeom wgm;
            bool pipe_ok = pipe_geometry(p->nq, N, tabd(PIPE_BLOCK / 64), heavy_rows, tw.rpw, tw.sub, tw.gram_global, tw.eager, p->n_reps, n_cus, &pg, contrib_doubles) == 0;
            bool wg_ok = !wide_q && wg_geometry(p->nq, N, tabd(WG_MAX_WAVES), WG_MAX_WAVES, &wgm) == 0;
            // MCSAS_EXEC_AUTO never picks a mode whose working set does not fit the device: the speculative modes
            // NEED their row cache (N + 2 windows of rows per chain) and the pipeline its window buffers on top (d rows, Gram blocks,
            // scalars, proposals: 2 Kb (qpad + W + 4 + P) doubles per chain) — against half of what is free, the same rule the
            // allocation (alloc_rows) applies; one wavefront per chain runs without a cache when it must.  An explicitly requested
            // mode still fails with MCSAS_ENOMEM.
            if (free_bytes != SIZE_MAX) {
                const double Rd = (double)p->n_reps, row = 8.0 * (double)qpad, fr = (double)free_bytes;
                if (pipe_ok) {
                    const double need = Rd * (((double)N + 2.0 * pg.kb + 1.0) * row
                                              + 2.0 * pg.kb * (row + 8.0 * (pg.w + 4 + MCSAS_MAX_ACTIVE) + 4.0));
                    if (need >= 0.5 * fr) pipe_ok = false;
                }
                if (wg_ok && Rd * ((double)N + 2.0 * wgm.window + 1.0) * row >= 0.5 * fr) wg_ok = false;
            }
            if (!heavy_rows) {
                // rows without an integral: the mode with the highest MEASURED rate at the nearest swept shape
                // (auto_table.h: 128..1024 q slots x 200..1000 contributions x 64..3000 repetitions on a 256-CU MI355X;
                // profiles/r03_mode_sweep*.jsonl).  Fewer than 64 chains: the pipeline wins at every swept shape (1, 10, 50
                // repetitions).  A device with another CU count is asked at the repetition count that loads it the same.
                mode = auto_mode_light(qpad, N, (double)p->n_reps * 256.0 / (double)n_cus, pipe_ok, wg_ok);
            } else {
                // Rows that cost an integral each: the pipeline at every chain count, since its producer waves pull the rows from a
                // queue (round 4, tools/sweep_heavy_modes2.sh, profiles/r04_heavy_modes.txt; steps/s pipeline | one wavefront per chain:
                // cylinders 5.2e6 | 1.3e6 at 300 chains, 6.0e6 | 3.6e6 at 2048, 5.7e6 | 4.4e6 at 4096; Kholodenko 4.4e6 | 0.9e6 at 300,
                // 5.2e6 | 4.8e6 at 2048, 4.7e6 | 4.5e6 at 4096; core-shell ellipsoids 2.5e6 | 0.7e6 at 300 chains x 1000 steps,
                // 3.8e6 | 3.6e6 at 2048 x 3000; the workgroup mode in between at best).  Where the pipeline's geometry does not fit
                // (fewer than 16 contributions), the older rule: one wavefront per chain from where the chains alone fill the
                // SIMDs, a workgroup per chain below.  Units of a 256-CU device.
                const double r_eff = (double)p->n_reps * 256.0 / (double)n_cus;
                if (pipe_ok) mode = MCSAS_EXEC_PIPELINE;
                else if (r_eff >= 1024.) mode = MCSAS_EXEC_WAVE;
                else if (wg_ok) mode = MCSAS_EXEC_WORKGROUP;
                else mode = MCSAS_EXEC_WAVE;
            }
        }
    }
    if (wide) { mode = MCSAS_EXEC_WORKGROUP; waves = wide_waves; }
    else if (wide_q) mode = MCSAS_EXEC_WAVE;
    if (mode == MCSAS_EXEC_WORKGROUP && waves < 2) waves = WG_MAX_WAVES;
    if (mode != MCSAS_EXEC_WORKGROUP) waves = 1;
    if (mode < MCSAS_EXEC_WAVE || mode > MCSAS_EXEC_PIPELINE) return fail(MCSAS_EINVAL, "exec_mode %d", mode);

    // per-contribution intensity rows: the speculative kernels add two windows of spare row slots
    int cache_rows = N;
    if (wide) {
        // q-split workgroup: no speculation, rows [N][qpad] like the wave kernel
    } else if (mode == MCSAS_EXEC_WORKGROUP) {
        if (wg_geometry(p->nq, N, tabd(waves), waves, &s->wg))
            return fail(MCSAS_EINVAL, "workgroup kernel: needs 2*window <= n_contrib and the window in LDS (nq=%d, n_contrib=%d, waves=%d)", p->nq, N, waves);
        cache_rows = N + 2 * s->wg.window;
    } else if (mode == MCSAS_EXEC_PIPELINE) {
        if (const int rcg = pipe_geometry(p->nq, N, tabd(PIPE_BLOCK / 64), heavy_rows, tw.rpw, tw.sub, tw.gram_global, tw.eager, p->n_reps, n_cus, &s->pipe, contrib_doubles)) {
            if (rcg == 2) return fail(MCSAS_EINVAL, "pipeline: the window's row buffers / proposal records do not fit the 160 KB of LDS (nq=%d, n_contrib=%d)", p->nq, N);
            return fail(MCSAS_EINVAL, "pipeline: needs n_contrib >= 16 and nq <= 1024 (nq=%d, n_contrib=%d)", p->nq, N);
        }
        cache_rows = N + 2 * s->pipe.kb;
    }
    s->qpl = qpl; s->qpad = qpad; s->wide = wide; s->waves = waves; s->mode = mode; s->cache_rows = cache_rows;
    return MCSAS_OK;
}

void fill_chain_settings(const mcsas_problem *p, ChainArgs *a) {
    a->n_contrib = p->n_contrib; a->n_reps = p->n_reps;
    a->find_bg = p->find_background != 0; a->pos_bg = p->positive_background != 0;
    a->start_from_min = p->start_from_minimum != 0; a->max_retries = p->max_retries;
    a->max_iter = p->max_iter; a->conv_crit = p->conv_crit;
    for (int c = 0; c < MCSAS_MAX_ACTIVE; ++c) {
        a->gen_lo[c] = p->gen_lo[c]; a->gen_hi[c] = p->gen_hi[c]; a->start_value[c] = p->start_value[c];
        a->gen_kind[c] = p->gen_kind[c];
    }
    a->seed = p->seed; a->rep_offset = p->rep_offset;
}

WeighedSums weigh_points(const double *I, const double *sigma, int n, double *w, double *wI, double *Iout) {
    WeighedSums s{0, 0, 0, 0};
    for (int i = 0; i < n; ++i) {
        const double e = sigma[i] == 0.0 ? 1.0 : sigma[i], wi = 1.0 / (e * e);
        w[i] = wi; wI[i] = wi * I[i]; Iout[i] = I[i];
        s.Sw += wi; s.SI += wi * I[i]; s.SII += wi * I[i] * I[i]; s.Ssig2 += e * e;
    }
    return s;
}

// ------------------------------------------------------------------------------ one population fitted to several data sets
int check_sets_request(const mcsas_problem *p, int32_t n_sets, const int32_t *set_nq, const mcsas_result *res,
                       const mcsas_sets_result *sets, SetsLayout *L, ModelArgs *margs, int32_t scale_mode) {
    const char *const who = "analyse_sets";
    if (!p || !res || !sets || !set_nq) return fail(MCSAS_EINVAL, "%s: null argument", who);
    if (p->struct_size != sizeof(mcsas_problem))
        return fail(MCSAS_EINVAL, "%s: mcsas_problem size %u, library expects %zu (ABI mismatch)", who, p->struct_size, sizeof(mcsas_problem));
    if (res->struct_size != sizeof(mcsas_result)) return fail(MCSAS_EINVAL, "%s: mcsas_result size mismatch", who);
    if (sets->struct_size != sizeof(mcsas_sets_result))
        return fail(MCSAS_EINVAL, "%s: mcsas_sets_result size %u, library expects %zu", who, sets->struct_size, sizeof(mcsas_sets_result));
    if (n_sets < 1 || n_sets > MCSAS_MAX_SETS) return fail(MCSAS_EINVAL, "%s: n_sets %d (1..%d)", who, (int)n_sets, MCSAS_MAX_SETS);
    if (sets->n_sets != n_sets) return fail(MCSAS_EINVAL, "%s: mcsas_sets_result.n_sets %d, the call's n_sets is %d", who, (int)sets->n_sets, (int)n_sets);
    if (scale_mode != MCSAS_SETS_SCALE_PER_SET && scale_mode != MCSAS_SETS_SCALE_SHARED)
        return fail(MCSAS_EINVAL, "%s: unknown scale_mode %d (%d: a scale per set, %d: one scale shared by the sets)", who, (int)scale_mode,
                    MCSAS_SETS_SCALE_PER_SET, MCSAS_SETS_SCALE_SHARED);
    if (p->reserved0) return fail(MCSAS_EINVAL, "%s: mcsas_problem.reserved0 must be 0 (it is %d)", who, p->reserved0);
    if (p->nq < 1 || !p->q || !p->intensity || !p->sigma) return fail(MCSAS_EINVAL, "%s: nq/q/intensity/sigma missing", who);
    if (p->n_active == 0)
        return fail(MCSAS_EINVAL, "%s: n_active == 0: without an active parameter there is no chain (mcsas_hip_analyse answers that case for one set)", who);
    if (p->model_id == -1) return fail(MCSAS_EINVAL, "%s: a host model (model_id -1: rows evaluated by the caller) is not supported", who);
    if (is_plugin_model(p->model_id)) return fail(MCSAS_EINVAL, "%s: a model plug-in (model_id %d) is not supported; built-in models only", who, p->model_id);
    if (p->model_id < 0 || p->model_id >= MCSAS_MODEL_COUNT) return fail(MCSAS_EINVAL, "%s: unknown model_id %d", who, p->model_id);
    if (p->exec_mode != MCSAS_EXEC_AUTO && p->exec_mode != MCSAS_EXEC_WAVE)
        return fail(MCSAS_EINVAL, "%s: exec_mode %d (%s) asked; several sets run one wavefront per chain (exec_mode 0 or %d)", who, p->exec_mode, exec_mode_name(p->exec_mode), MCSAS_EXEC_WAVE);
    if (p->n_devices > 1) return fail(MCSAS_EINVAL, "%s: n_devices %d: a device list is not supported, the call runs on one device", who, p->n_devices);
    if (p->positive_background) return fail(MCSAS_EINVAL, "%s: positive_background is not supported with several sets", who);
    if (p->smear_nk > 0) return fail(MCSAS_EINVAL, "%s: smearing (smear_nk %d) is not supported with several sets", who, p->smear_nk);
    if (p->cache_intensities == 0) return fail(MCSAS_EINVAL, "%s: cache_intensities == 0: the kernel keeps every contribution's row (cached rows only)", who);
    if (p->n_contrib < 1 || p->n_reps < 1) return fail(MCSAS_EINVAL, "%s: n_contrib and n_reps must be >= 1", who);
    if (p->max_iter < 0 || p->max_retries < 0) return fail(MCSAS_EINVAL, "%s: max_iter/max_retries negative", who);
    if (p->replay_stream && p->replay_len < 1) return fail(MCSAS_EINVAL, "%s: replay_len must be >= 1", who);
    for (int c = 0; c < p->n_active && c < MCSAS_MAX_ACTIVE; ++c)
        if (p->gen_kind[c] < MCSAS_GEN_UNIFORM || p->gen_kind[c] > MCSAS_GEN_EXP3) return fail(MCSAS_EINVAL, "%s: gen_kind[%d]=%d", who, c, p->gen_kind[c]);

    *L = SetsLayout{};
    L->S = n_sets; L->scale_mode = scale_mode;
    long long sum = 0, slot_sum = 0;
    for (int s = 0; s < n_sets; ++s) {
        if (set_nq[s] < 3) return fail(MCSAS_EINVAL, "%s: set %d has %d points; every set needs at least 3", who, s, (int)set_nq[s]);
        sum += set_nq[s]; slot_sum += ((long long)set_nq[s] + WAVE - 1) / WAVE;
    }
    if (sum != p->nq) return fail(MCSAS_EINVAL, "%s: sum of set_nq %lld != nq %d", who, sum, p->nq);
    if (slot_sum > SETS_MAX_SLOTS)
        return fail(MCSAS_EINVAL, "%s: the sets padded to whole slots of %d take %lld padded slots (%lld entries) > %d (%d entries)", who, WAVE, slot_sum,
                    slot_sum * WAVE, SETS_MAX_SLOTS, SETS_MAX_SLOTS * WAVE);
    for (int s = 0, o = 0, k = 0; s < n_sets; ++s) {
        L->nq[s] = set_nq[s]; L->off[s] = o; L->slots[s] = (set_nq[s] + WAVE - 1) / WAVE; L->pad_off[s] = k * WAVE;
        o += set_nq[s]; k += L->slots[s];
        L->end_mask |= 1u << (k - 1);
        L->total_slots = k;
    }
    for (L->qpl = 1; L->qpl < L->total_slots;) L->qpl *= 2;
    if (int rc = fill_model_args(p, margs)) return rc;
    L->lds_bytes = sizeof(double) * (SETS_LDS_DOUBLES + 4 * (size_t)L->qpl * WAVE + table_doubles_block(p->model_id, margs->int_div, 1));
    if (L->lds_bytes > 160 * 1024) return fail(MCSAS_EINVAL, "%s: LDS need %zu B > 160 KiB", who, L->lds_bytes);
    return MCSAS_OK;
}

void lay_out_sets(const mcsas_problem *p, const SetsLayout &L, SetsData *d, SetsArgs *sa) {
    const size_t qpad = (size_t)L.qpl * WAVE;
    d->q.assign(qpad, p->q[0]); d->w.assign(qpad, 0.); d->wI.assign(qpad, 0.); d->I.assign(qpad, 0.);
    memset(sa, 0, sizeof *sa);
    sa->n_sets = L.S; sa->end_mask = L.end_mask; sa->scale_mode = L.scale_mode;
    for (int s = 0; s < L.S; ++s) {
        const int src = L.off[s], dst = L.pad_off[s];
        std::fill_n(&d->q[dst], L.slots[s] * WAVE, p->q[src]);
        std::copy_n(p->q + src, L.nq[s], &d->q[dst]);
        const WeighedSums t = weigh_points(p->intensity + src, p->sigma + src, L.nq[s], &d->w[dst], &d->wI[dst], &d->I[dst]);
        // (1 / Sw, SI / Sw, SII - SI² / Sw: the operations of chain_body.inc, unfused here as there)
        sa->set[s] = SetConst{t.Sw, t.SI, t.SII, 1.0 / t.Sw, t.SI / t.Sw, t.SII - t.SI * t.SI / t.Sw, (double)L.nq[s]};
    }
}

// ------------------------------------------------------------------------------ the histogram of a joint fit
int check_hist_sets_request(const mcsas_problem *p, int32_t n_sets, const int32_t *set_nq, int32_t scale_mode, int32_t ref_set,
                            uint32_t visible_sets, const mcsas_sets_result *sets, int32_t off[MCSAS_MAX_SETS + 1]) {
    const char *const who = "histogram_sets";
    if (!p || !set_nq || !sets) return fail(MCSAS_EINVAL, "%s: null argument", who);
    if (p->struct_size != sizeof(mcsas_problem))
        return fail(MCSAS_EINVAL, "%s: mcsas_problem size %u, library expects %zu (ABI mismatch)", who, p->struct_size, sizeof(mcsas_problem));
    if (sets->struct_size != sizeof(mcsas_sets_result))
        return fail(MCSAS_EINVAL, "%s: mcsas_sets_result size %u, library expects %zu", who, sets->struct_size, sizeof(mcsas_sets_result));
    if (n_sets < 1 || n_sets > MCSAS_MAX_SETS) return fail(MCSAS_EINVAL, "%s: n_sets %d (1..%d)", who, (int)n_sets, MCSAS_MAX_SETS);
    if (sets->n_sets != n_sets) return fail(MCSAS_EINVAL, "%s: mcsas_sets_result.n_sets %d, the call's n_sets is %d", who, (int)sets->n_sets, (int)n_sets);
    if (!sets->scaling || !sets->background) return fail(MCSAS_EINVAL, "%s: mcsas_sets_result.scaling and .background receive every set's fit; one is NULL", who);
    long long sum = 0;
    for (int s = 0; s < n_sets; ++s) {
        if (set_nq[s] < 3) return fail(MCSAS_EINVAL, "%s: set %d has %d points; every set needs at least 3", who, s, (int)set_nq[s]);
        sum += set_nq[s];
    }
    if (sum != p->nq) return fail(MCSAS_EINVAL, "%s: sum of set_nq %lld != nq %d", who, sum, p->nq);
    if (ref_set < 0 || ref_set >= n_sets) return fail(MCSAS_EINVAL, "%s: ref_set %d: there are %d sets", who, (int)ref_set, (int)n_sets);
    if (visible_sets == 0) return fail(MCSAS_EINVAL, "%s: visible_sets is empty: no set's points would judge what is visible", who);
    if (visible_sets >> n_sets) return fail(MCSAS_EINVAL, "%s: visible_sets 0x%x names a set that is not there (%d sets)", who, visible_sets, (int)n_sets);
    if (scale_mode != MCSAS_SETS_SCALE_PER_SET && scale_mode != MCSAS_SETS_SCALE_SHARED)
        return fail(MCSAS_EINVAL, "%s: unknown scale_mode %d (%d: a scale per set, %d: one scale shared by the sets)", who, (int)scale_mode,
                    MCSAS_SETS_SCALE_PER_SET, MCSAS_SETS_SCALE_SHARED);
    if (p->positive_background) return fail(MCSAS_EINVAL, "%s: positive_background is not supported with several sets", who);
    if (p->smear_nk != 0 || p->smear_locs || p->smear_q_offset || p->smear_weights)
        return fail(MCSAS_EINVAL, "%s: smearing (smear_nk %d) is not supported with several sets", who, p->smear_nk);
    if (p->model_id == -1) return fail(MCSAS_EINVAL, "%s: a host model (model_id -1: rows evaluated by the caller) is not supported", who);
    if (is_plugin_model(p->model_id)) return fail(MCSAS_EINVAL, "%s: a model plug-in (model_id %d) is not supported; built-in models only", who, p->model_id);
    if (p->model_id < 0 || p->model_id >= MCSAS_MODEL_COUNT) return fail(MCSAS_EINVAL, "%s: unknown model_id %d", who, p->model_id);
    int o = 0;
    for (int s = 0; s <= MCSAS_MAX_SETS; ++s) {
        off[s] = o;
        if (s < n_sets) o += set_nq[s];
    }
    return MCSAS_OK;
}

// ------------------------------------------------------------------------------ what a start and a trace are refused for
// the first non-finite value of the columns [first, first + R) of start[N][P][stride], or MCSAS_OK
int check_start_finite(const char *who, const double *start, size_t N, size_t P, size_t stride, size_t first, size_t R) {
    for (size_t i = 0; i < N * P; ++i)
        for (size_t r = 0; r < R; ++r)
            if (!std::isfinite(start[i * stride + first + r]))
                return fail(MCSAS_EINVAL, "%s: start[%zu][%zu][%zu] (index %zu) is not finite", who, i / P, i % P, first + r, i * stride + first + r);
    return MCSAS_OK;
}

const char *exec_mode_name(int mode) {
    return mode == MCSAS_EXEC_WAVE ? "MCSAS_EXEC_WAVE" : mode == MCSAS_EXEC_WORKGROUP ? "MCSAS_EXEC_WORKGROUP" : mode == MCSAS_EXEC_PIPELINE ? "MCSAS_EXEC_PIPELINE" : "MCSAS_EXEC_AUTO";
}

int check_trace_arrays(const char *who, const mcsas_trace *tr) {
    if (!tr) return fail(MCSAS_EINVAL, "%s: trace is NULL", who);
    if (tr->struct_size != sizeof(mcsas_trace)) return fail(MCSAS_EINVAL, "%s: mcsas_trace size %u, library expects %zu", who, tr->struct_size, sizeof(mcsas_trace));
    if (tr->capacity < 1) return fail(MCSAS_EINVAL, "%s: trace capacity %d (>= 1)", who, (int)tr->capacity);
    if (!tr->count || !tr->chisq0 || !tr->step || !tr->chisq || !tr->values)
        return fail(MCSAS_EINVAL, "%s: trace array %s is NULL", who, !tr->count ? "count" : !tr->chisq0 ? "chisq0" : !tr->step ? "step" : !tr->chisq ? "chisq" : "values");
    return MCSAS_OK;
}

// ------------------------------------------------------------------------------ how a kernel family is launched and named
unsigned family_block(KernelFamily family, int waves) {
    const FamilyInfo::Block b = KERNEL_FAMILY[family].block;
    return b == FamilyInfo::BLOCK_PIPE ? PIPE_BLOCK : (b == FamilyInfo::BLOCK_WAVES ? WAVE * waves : WAVE);
}

int plugin_kernel_name(int model_id, KernelFamily family, int qpl, bool flag, bool given, std::string *expr, std::string *key) {
    const FamilyInfo &f = KERNEL_FAMILY[family];
    if (given && !f.startable) return fail(MCSAS_EINVAL, "no %s start kernel for model %d qpl %d", f.key, model_id, qpl);
    *expr = std::string("mcsas::") + f.kernel + "<MCSAS_MODEL_PLUGIN, " + std::to_string(qpl) + (f.flagged ? (flag ? ", true" : ", false") : "")
            + (f.startable ? (given ? ", true" : ", false") : "") + ">";
    *key = std::string(f.key) + (given ? " start " : " ") + std::to_string(qpl) + (f.flagged ? (flag ? " 1" : " 0") : "");
    return MCSAS_OK;
}

// ------------------------------------------------------------------------------ a fetched trace block, a pipeline launch's ticks
void trace_transpose(const char *block, size_t R, size_t K, size_t P, const ChainOut *out, mcsas_trace *tr) {
    const TraceLayout at(R, K, P);
    const int64_t *hstep = (const int64_t *)(block + at.step);
    const double *hchi = (const double *)(block + at.chisq), *hval = (const double *)(block + at.values);
    const double *hchi0 = (const double *)(block + at.chisq0);
    const double nan = std::nan("");
    for (size_t r = 0; r < R; ++r) {
        const int64_t moves = out[r].num_moves;
        tr->count[r] = moves; tr->chisq0[r] = hchi0[r];
        for (size_t i = 0; i < K; ++i) {
            const bool kept = (int64_t)i < moves;
            tr->step[i * R + r] = kept ? hstep[r * K + i] : -1;
            tr->chisq[i * R + r] = kept ? hchi[r * K + i] : nan;
            for (size_t p = 0; p < P; ++p) tr->values[(i * P + p) * R + r] = kept ? hval[(r * K + i) * P + p] : nan;
        }
    }
}

long long pipeline_tick_budget(int64_t max_iter, int32_t max_retries, int Kb) {
    const long long TICK_CAP = 2000000000LL;
    const long long win_per_attempt = (long long)(max_iter / Kb) + 4;
    const long long attempts = (long long)max_retries + 1;
    const long long one_attempt = std::min((long long)((max_iter + Kb - 1) / Kb) + 1, TICK_CAP);
    return attempts == 1 ? one_attempt
                         : ((win_per_attempt >= TICK_CAP / attempts) ? TICK_CAP : std::min(attempts * win_per_attempt + 4, TICK_CAP));
}
