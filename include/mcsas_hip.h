/* mcsas_hip.h — C ABI of the MI355X-native McSAS Monte-Carlo core (libmcsas_hip.so).
 *
 * This is the drop-in boundary.  The reference has no FFI; the path it replaces is
 * the pure-Python call chain
 *     McSAS.analyse()                         src/mcsas/mcsas/mcsas.py:191-285
 *       -> McSAS.mcFit()                      src/mcsas/mcsas/mcsas.py:287-439
 *            -> ScatteringModel.calc()        src/mcsas/bases/model/scatteringmodel.py:79-109
 *            -> BackgroundScalingFit.calc()   src/mcsas/mcsas/backgroundscalingfit.py:112-139
 *            -> ScatteringModel.generateParameters()  src/mcsas/bases/model/scatteringmodel.py:117-127
 * Every entry point below names the reference interface it stands in for.  Plain pointers and
 * sizes only; all arrays are caller-owned host memory, double = IEEE binary64, C order.
 * All functions return 0 on success or a negative MCSAS_E* code and never throw; the message of
 * the last failure on the calling thread is available from mcsas_hip_last_error().
 * One in-flight call per plan (mirrors the reference's non-reentrant model objects).
 */
#ifndef MCSAS_HIP_H
#define MCSAS_HIP_H

#ifndef __HIPCC_RTC__   /* (the library's run-time compiler has the fixed-width types built in) */
#include <stdint.h>
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define MCSAS_ABI_VERSION 5
#define MCSAS_MAX_ACTIVE 4   /* active (fitted) parameters per contribution: columns of rset */
#define MCSAS_MAX_PARAMS 8   /* full parameter vector of a model */
#define MCSAS_MAX_DEVICES 16 /* devices one mcsas_hip_analyse call may spread its repetitions over */

/* model_id: which ScatteringModel.formfactor/volume/absVolume/surface set is evaluated.
 * Parameter vector order = the reference's `parameters` tuple of that class. */
enum {
    MCSAS_MODEL_SPHERE = 0,      /* models/sphere.py:12-63            (radius, sld) */
    MCSAS_MODEL_CYL_ISO = 1,     /* models/cylindersisotropic.py:17-101 (radius, useAspect, length, aspect, intDiv, sld) */
    MCSAS_MODEL_ELL_CS = 2,      /* models/ellipsoidalcoreshell.py:14-97 (a, b, t, eta_c, eta_s, eta_sol, intDiv) */
    MCSAS_MODEL_KHOLODENKO = 3,  /* models/kholodenko.py:51-94         (radius, lenKuhn, lenContour) */
    MCSAS_MODEL_ELL_ISO = 4,     /* models/ellipsoidsisotropic.py:18-84 (a, useAspect, c, aspect, intDiv, sld) */
    MCSAS_MODEL_SPH_CS = 5,      /* models/sphericalcoreshell.py:14-77 (radius, t, eta_c, eta_s, eta_sol) */
    MCSAS_MODEL_GAUSS_CHAIN = 6, /* models/gaussianchain.py:14-66      (rg, bp, etas, k) */
    MCSAS_MODEL_LMA_SPHERE = 7,  /* models/lmadensesphere.py:14-106    (radius, volFrac, mf, sld) */
    MCSAS_MODEL_COUNT = 8,
    MCSAS_MODEL_PLUGIN = 8,      /* the template slot run-time plug-ins are compiled into (csrc/plugin_model.h); never a caller's model_id */
    MCSAS_MODEL_PLUGIN0 = 64     /* first id mcsas_hip_plugin_compile hands out */
};
#define MCSAS_MAX_PLUGINS 32 /* plug-in models a process may register */

/* gen_kind: NumberGenerator subclass of an active parameter (bases/algorithm/numbergenerator.py) */
enum {
    MCSAS_GEN_UNIFORM = 0,  /* RandomUniform       :28-31   u */
    MCSAS_GEN_EXP1 = 1,     /* RandomExponential   :168-175 (10^u - 1)/10 */
    MCSAS_GEN_EXP2 = 2,     /* RandomExponential2  :181-184 (10^(2u) - 1)/100 */
    MCSAS_GEN_EXP3 = 3      /* RandomExponential3  :186-189 (10^(3u) - 1)/1000 */
};

/* exec_mode: how chains are mapped onto the chip.  Every mode replays the reference's trajectories decision for decision
 * (tests/test_parity_gpu.py); the modes sum the same terms in different orders, so two FREE-RUNNING chains with the same
 * seed can take different turns at a numerically tied step (replacing one negligible contribution by another moves chi²
 * by less than its rounding error).  A repetition's result is reproducible for the same mode, whatever the number of
 * repetitions or devices beside it: nothing a chain decides depends on how many chains share a launch (the pipeline's window
 * is fixed for rows without an integral; for rows with an integral it follows the chain count, and the decisions are kept
 * independent of it: csrc/chain_pipe.h, PipeGeom::resum_every).
 * q-points (the reference takes any data.count, mcsas.py:210): up to 1024 in every mode; 1025..16384 (un-binned data files,
 * nBin = 0) one workgroup per chain with the q-points split over its waves (csrc/chain_wide.h: MCSAS_EXEC_WORKGROUP, and
 * what MCSAS_EXEC_AUTO picks); up to 4096 MCSAS_EXEC_WAVE also runs; beyond 16384 MCSAS_EINVAL. */
enum {
    MCSAS_EXEC_AUTO = 0,
    MCSAS_EXEC_WAVE = 1,      /* one wavefront per chain: many repetitions (>= ~1000) */
    MCSAS_EXEC_WORKGROUP = 2, /* one workgroup per chain: speculative proposal window in LDS (nq <= 1024), q-split (nq > 1024) */
    MCSAS_EXEC_PIPELINE = 3   /* producer kernels on every CU + one scan workgroup per chain: few repetitions (nq <= 1024) */
};

enum {
    MCSAS_OK = 0,
    MCSAS_EINVAL = -1,      /* bad argument / unsupported size */
    MCSAS_ENODEV = -2,      /* no usable HIP device */
    MCSAS_EHIP = -3,        /* HIP runtime error (see mcsas_hip_last_error) */
    MCSAS_ENOMEM = -4,
    MCSAS_ESTREAM = -5,     /* replay stream shorter than the draws a chain consumed */
    MCSAS_ECALLBACK = -6    /* the caller's rows callback reported a failure (mcsas_hip_analyse_host_rows) */
};

/* Everything McSAS.analyse() reads from self.data, self.model and the algorithm settings. */
typedef struct mcsas_problem {
    uint32_t struct_size;        /* sizeof(mcsas_problem), ABI check */
    int32_t  model_id;           /* MCSAS_MODEL_* */

    /* data: SASData.q, data.f.binnedData, data.f.binnedDataU (dataobj/sasdata.py:51-55,
     * backgroundscalingfit.py:113-117; sigma == 0 is treated as 1 like the reference). SI units. */
    int32_t  nq;
    const double *q;
    const double *intensity;
    const double *sigma;

    /* model: values of ALL parameters (inactive ones are used as they are) + the active set */
    double   params[MCSAS_MAX_PARAMS];
    int32_t  n_active;                           /* model.activeParamCount() */
    int32_t  active_index[MCSAS_MAX_ACTIVE];     /* ascending indices into params[] (activeParams() order) */
    double   gen_lo[MCSAS_MAX_ACTIVE];           /* activeRange ∩ valueRange (utils/parameter.py:715-728, */
    double   gen_hi[MCSAS_MAX_ACTIVE];           /*   bases/algorithm/parameter.py:66-84) */
    int32_t  gen_kind[MCSAS_MAX_ACTIVE];         /* MCSAS_GEN_* */
    double   clip_lo[MCSAS_MAX_ACTIVE];          /* valueRange: Parameter.setValue clips into it */
    double   clip_hi[MCSAS_MAX_ACTIVE];          /*   (bases/algorithm/parameter.py:405-414,489-495) */
    double   start_value[MCSAS_MAX_ACTIVE];      /* startFromMinimum fill value (mcsas.py:310-315) */

    /* algorithm settings (mcsas/mcsasparameters.json) */
    int32_t  n_contrib;          /* numContribs */
    int32_t  n_reps;             /* numReps handled by THIS call (a shard when multi-GPU) */
    int64_t  max_iter;           /* maxIterations */
    double   comp_exp;           /* compensationExponent */
    double   conv_crit;          /* convergenceCriterion */
    int32_t  max_retries;        /* maxRetries: up to max_retries+1 attempts per rep (mcsas.py:220-246) */
    int32_t  find_background;    /* findBackground */
    int32_t  positive_background;
    int32_t  start_from_minimum;

    /* random numbers.  Free-running: Philox4x32-10 keyed by `seed`, one independent stream per
     * chain id (rep_offset + local rep).  Replay: replay_stream != NULL supplies, per rep, the
     * raw uniforms numpy.random.uniform would have returned, consumed in the reference's order
     * (N draws per active parameter at chain start, then n_active per step; retries continue). */
    uint64_t seed;
    int32_t  rep_offset;         /* global index of this shard's first rep */
    int32_t  reserved0;          /* must be 0: MCSAS_EINVAL otherwise */
    const double *replay_stream; /* [n_reps][replay_len] or NULL */
    int64_t  replay_len;

    /* cooperative stop (McSAS.stop, mcsas.py:357): polled by the host while the kernel runs and
     * forwarded to the device; may be NULL */
    const volatile int32_t *stop;

    /* execution */
    int32_t  device;             /* HIP device ordinal, -1 = current device */
    int32_t  waves_per_chain;    /* 0 = auto; 1 = one wavefront per chain; >1 = workgroup per chain */
    int32_t  cache_intensities;  /* -1 auto, 0 re-evaluate `old` every step like mcsas.py:362, 1 keep rows in HBM */
    int32_t  exec_mode;          /* MCSAS_EXEC_*: 0 auto, 1 wavefront per chain, 2 workgroup per chain, 3 whole-chip pipeline */

    /* beam-profile smearing (ABI 2): what SASConfig.prepareSmearing left in data.locs and
     * data.config.smearing.prepared (dataobj/sasconfig.py:308-339, dataobj/sasdata.py:165).  With
     * smear_nk > 0 and a model whose class has canSmear = True (Sphere, LMADenseSphere) every
     * calcIntensity is 2 * trapz(F(locs)^2 * w * weights, x = q_offset) (bases/model/sasmodel.py:56-73);
     * other models ignore it, as in the reference.  smear_nk = 0: off. */
    int32_t  smear_nk;               /* integration points per q (nSteps + 1, or 2 ceil(nSteps/2) + 1) */
    int32_t  reserved1;
    const double *smear_locs;        /* [nq][smear_nk], row-major: where F is evaluated */
    const double *smear_q_offset;    /* [smear_nk] */
    const double *smear_weights;     /* [smear_nk] beam-profile weights */

    /* several GPUs (ABI 3).  The repetition loop of McSAS.analyse (mcsas.py:214-262) is a serial `for nr in
     * range(numReps)` over chains that share nothing but read-only data; with n_devices > 1 mcsas_hip_analyse runs
     * contiguous blocks of repetitions on devices[0..n_devices) at the same time (one host thread, one plan and one
     * stream per device; blocks differ by at most one repetition) and writes every block into the caller's arrays
     * at its place.  The chain id of a repetition is rep_offset + its index whatever the split, so a repetition's
     * random stream does not depend on the device count — and neither does its result as long as every block
     * runs in the same execution mode (set exec_mode; MCSAS_EXEC_AUTO looks at the block's own repetition count).
     * n_devices = 0 or 1: `device` alone.  A device may be listed more than once.  Plans take `device` only. */
    int32_t  n_devices;
    int32_t  devices[MCSAS_MAX_DEVICES];
    int32_t  reserved2;
} mcsas_problem;

/* What mcFit returns per repetition (mcsas.py:428-439) gathered the way analyse() stores it
 * (mcsas.py:203-210,233-251).  Caller allocates every non-NULL array. */
typedef struct mcsas_result {
    uint32_t struct_size;
    uint32_t reserved;
    double  *contribs;     /* [n_contrib][n_active][n_reps]  == contributions, mcsas.py:203-205 */
    double  *fit;          /* [nq][n_reps]                   == contribMeasVal[0], mcsas.py:210 */
    double  *chisq;        /* [n_reps] final reduced chi-squared (conval) */
    double  *scaling;      /* [n_reps] details['scaling'] */
    double  *background;   /* [n_reps] details['background'] */
    int64_t *num_iter;     /* [n_reps] details['numIterations'] of the last attempt */
    int64_t *num_moves;    /* [n_reps] details['numMoves'] */
    int32_t *attempts;     /* [n_reps] mcFit calls made for this rep */
    int32_t *converged;    /* [n_reps] chisq <= conv_crit */
    double  *seconds;      /* [n_reps] device wall time of the chain, all attempts */
    int64_t *draws;        /* [n_reps] uniforms consumed (replay bookkeeping); may be NULL */
} mcsas_result;

/* ---- one-shot: replaces McSAS.analyse()'s repetition loop (mcsas.py:214-262) ----------------
 * n_active == 0 (no active fit parameter, mcsas.py:198-201, 238-239, 322-323): the reference runs ONE
 * repetition of ONE contribution and mcFit returns the model intensity at the fixed parameter values;
 * here: fit[nq] = that intensity, chisq[0] = -1, scaling[0] = 1, background[0] = 0, num_iter[0] = 0 — the
 * result arrays are then used as if n_contrib = n_reps = 1. */
int mcsas_hip_analyse(const mcsas_problem *problem, mcsas_result *result);
/* how mcsas_hip_analyse splits n_reps repetitions over n_devices devices: block `index` = repetitions
 * [*first, *first + *count) (contiguous, in device-list order, sizes differ by at most one; count may be 0) */
int mcsas_hip_shard(int32_t n_reps, int32_t n_devices, int32_t index, int32_t *first, int32_t *count);

/* ---- McSAS.analyse() for a model that exists only as HOST code (ABI 4) -------------------------------------------------
 * The reference's plug-in contract is a ScatteringModel subclass with Python formfactor() / volume() / absVolume() / surface()
 * (bases/model/scatteringmodel.py:16-58), evaluated one parameter set at a time by ScatteringModel.calc (:79-105: p.setValue(v)
 * on every active parameter — which clips into the valueRange —, then calcIntensity, bases/model/sasmodel.py:46-79), found by
 * FindModels in any file under models/ (utils/findmodels.py:120-186).  Such a model has no device code.  A proposal depends on the random
 * stream only, never on the state of its chain (mcsas.py:358), so the library draws the proposals of the next `window` steps of
 * every chain on the host (the same counter-based / replayed streams and generator transforms as every other entry point), hands
 * ALL of them to `rows_cb` in one call, and runs everything else of McSAS.mcFit on the device (csrc/chain_feed.h): the row
 * cache (`old`, mcsas.py:362), test = ft - old + new, the scale / background fit and chi² (:376), the decisions (:379-390), the
 * final fit (:424-430); the retry loop of analyse() (:220-246) and McSAS.stop are followed between windows.
 *   rows_cb(user, n, pset, rows): pset[n][n_active] parameter sets (activeParams() order, NOT yet clipped: setValue does that)
 *     -> rows[n][nq] = calcIntensity(data, compensationExponent)[0] of each; return 0, anything else aborts with MCSAS_ECALLBACK.
 *     Called from the calling thread only, with 1 <= n <= max(n_contrib, window) * n_reps rows (bounded by ~256 MB of rows).
 *   window: proposals evaluated ahead per chain and call (< 1: 64); a chain that ends inside a window wastes the rest of it.
 * Uses problem->{nq, q, intensity, sigma, n_active, gen_*, start_value, n_contrib, n_reps, max_iter, conv_crit, max_retries,
 * find_background, positive_background, start_from_minimum, seed, rep_offset, replay_*, stop, device}; model_id, params, clip_*,
 * comp_exp and smear_* are the callback's business (calcIntensity smears by itself, sasmodel.py:56-73).  nq <= 16384.
 * result: as mcsas_hip_analyse; seconds[] = host wall time from the start of the call to the end of the repetition. */
typedef int (*mcsas_rows_callback)(void *user, int32_t n, const double *pset, double *rows);
int mcsas_hip_analyse_host_rows(const mcsas_problem *problem, mcsas_rows_callback rows_cb, void *user, int32_t window,
                                mcsas_result *result);

/* ---- the same, with the rows of a round produced ON THE DEVICE by the caller (additive to ABI 5) -------------------------
 * For a model the caller has as device code of its own (torch tensor lines, a kernel of a C caller): the proposals of a round are
 * generated on the device (csrc/chain_feed.h: feed_draw_kernel — the draw source, generator transform and expression of the chain
 * kernels, so the values are bit for bit those of MCSAS_EXEC_WAVE for the same seed or replay stream) straight into d_pset, the
 * caller fills the rows of the whole round in d_rows, and feed_rows_kernel decides on them where they lie.  Nothing of a round
 * crosses the bus but the round's metadata (up) and the chains' state (down).
 *   d_pset [capacity_rows][n_active], d_rows [capacity_rows][row_stride]: the CALLER's device memory on problem->device;
 *     row_stride = nq rounded up to 64.  The library zeroes d_rows once, at the start of the call.
 *   rows_cb(user, n): d_pset[0..n) holds the round's parameter sets (activeParams() order, NOT yet clipped), complete on the device
 *     when the callback is entered; the callback fills columns 0..nq of rows 0..n of d_rows and nothing else (the padding columns
 *     stay zero), complete on the device when it returns; return 0, anything else aborts with MCSAS_ECALLBACK.  Calling thread only.
 *   mcsas_hip_device_rows_shape (touches no device): *min_rows = max(n_contrib, window) is the least capacity_rows (one chain per
 *     round); *useful_rows = min(n_reps * min_rows, 256 MiB / (row_stride * 8)), never below min_rows, is the most a round uses;
 *     *row_stride as above.  window < 1: 64.  Any of the three may be NULL.
 * Refused before a device is touched: NULL problem / rows_cb / result / d_pset / d_rows, a wrong struct_size, capacity_rows <
 * min_rows, and everything mcsas_hip_analyse_host_rows refuses of a problem; after the device is selected: a buffer that is not
 * device memory of that device (MCSAS_EINVAL, no kernel is launched on it).  A failed host allocation: MCSAS_ENOMEM.
 * Everything else — the fields of problem that are read, the retry loop, stop, the replay rule (a draw behind the stream's end is
 * 0.5; MCSAS_ESTREAM only if a step a chain TOOK needed one), result — is mcsas_hip_analyse_host_rows.
 * Measured once (one MI355X, 2026-10-19; profiles/device_rows_ab.md): a Sphere typed as a Python model, 100 q x 200 contributions x
 * 10 repetitions x 20 000 steps, window 64: 8.81 us of wall time per step through mcsas_hip_analyse_host_rows (numpy), 0.438 us
 * through this entry point (the same model in torch), 20 times faster; the device run is bound by its rounds (0.28 ms each). */
typedef int (*mcsas_device_rows_callback)(void *user, int32_t n);
int mcsas_hip_device_rows_shape(const mcsas_problem *problem, int32_t window, int64_t *min_rows, int64_t *useful_rows,
                                int32_t *row_stride);
int mcsas_hip_analyse_device_rows(const mcsas_problem *problem, double *d_pset, double *d_rows, int64_t capacity_rows,
                                  mcsas_device_rows_callback rows_cb, void *user, int32_t window, mcsas_result *result);

/* ---- resident plan: same work split so that inputs/workspaces live in HBM across runs ------- */
typedef struct mcsas_plan mcsas_plan;
int  mcsas_hip_plan_create(const mcsas_problem *problem, mcsas_plan **plan);
/* enqueue all chains on `hip_stream` (a hipStream_t, NULL = default stream).  Wavefront / workgroup modes:
 * one asynchronous kernel launch.  Pipeline mode: one launch per window of steps; the call stays ahead of the
 * GPU by at most 64 launches and otherwise waits on an event (every 16 launches) while it forwards
 * problem->stop and watches for the last chain to finish — it returns when everything is ENQUEUED, which for
 * long runs is shortly before everything has run. */
int  mcsas_hip_plan_launch(mcsas_plan *plan, void *hip_stream);
/* wait for the launch (forwarding problem->stop meanwhile) and copy results out */
int  mcsas_hip_plan_fetch(mcsas_plan *plan, mcsas_result *result);
/* Result slots.  A plan keeps MCSAS_PLAN_SLOTS sets of what a finished analysis is read back from (parameter sets, fits,
 * per-chain outputs, timing events) over ONE set of workspaces, so that a series of analyses — one data set after the other,
 * gui/calc.py:271-330 — keeps the device busy: launch into slot 1 while slot 0 is being fetched and unpacked.  The slots of a
 * plan share its workspaces: launch them on the same stream (they then run one after the other).  mcsas_hip_plan_launch /
 * _fetch are slot 0; _last_ms and _total_steps report the slot fetched last. */
#define MCSAS_PLAN_SLOTS 2
int  mcsas_hip_plan_launch_slot(mcsas_plan *plan, void *hip_stream, int32_t slot);
int  mcsas_hip_plan_fetch_slot(mcsas_plan *plan, int32_t slot, mcsas_result *result);
/* device time of the last launch measured with HIP events on its stream, milliseconds */
int  mcsas_hip_plan_last_ms(mcsas_plan *plan, double *ms);
/* total MC steps executed by the last launch (sum of iterations over chains and attempts) */
int  mcsas_hip_plan_total_steps(mcsas_plan *plan, int64_t *steps);
/* how the plan executes: info[0] = exec mode chosen (MCSAS_EXEC_*), [1] = waves per chain, [2] = q slots
 * per lane, [3] = speculative window (steps), [4] = kernel launches of the last mcsas_hip_plan_launch,
 * [5] = 1 if per-contribution intensity rows are cached in HBM, [6..7] reserved */
int  mcsas_hip_plan_info(mcsas_plan *plan, int32_t info[8]);
/* change seed / rep_offset between launches without re-uploading anything else */
int  mcsas_hip_plan_reseed(mcsas_plan *plan, uint64_t seed, int32_t rep_offset);
void mcsas_hip_plan_destroy(mcsas_plan *plan);

/* ---- several analyses in one launch (ABI 5): a series of data sets (gui/calc.py:271-379) --------------------------------
 * A series fits the same model with the same settings to many data sets, each with a few repetitions: too few chains per
 * analysis to fill the chip one wavefront per chain.  The chains of different analyses share nothing, so a batch runs them
 * together: one launch of the wavefront-per-chain kernel per group of analyses with the same kernel (model, q slots per lane,
 * row cache), block b = one repetition of one analysis, reading that analysis' own argument block.
 * mcsas_hip_plan_launch_batch: enqueues the n resident plans on `hip_stream` (slot 0 of each; it first waits for any earlier
 *   analysis of a plan that is still in flight, as mcsas_hip_plan_launch does).  Every plan must be on the same device, must
 *   have resolved to MCSAS_EXEC_WAVE, and all must carry the same `stop` pointer (or all NULL); a plan may appear once.
 *   Otherwise MCSAS_EINVAL and nothing is launched.  The chains of the whole batch watch ONE stop word: a stop forwarded by
 *   the fetch of any plan of the batch ends every chain.  Afterwards each plan is fetched on its own (mcsas_hip_plan_fetch);
 *   _last_ms is the device time of its group's launch, _total_steps its own steps; mcsas_hip_plan_reseed between launches holds.
 * mcsas_hip_analyse_batch: the one-shot form: problems[i] -> results[i] (each sized as for mcsas_hip_analyse).  exec_mode AUTO
 *   means wave here; PIPELINE / WORKGROUP, n_devices > 1 or nq > 4096 give MCSAS_EINVAL before anything is launched.  A problem
 *   with n_active == 0 is answered at its place exactly as mcsas_hip_analyse answers it.
 * Contract: results[i] is IDENTICAL to mcsas_hip_analyse of problems[i] with exec_mode = MCSAS_EXEC_WAVE (same seed /
 * rep_offset / replay stream): contribs, fit, chisq, scaling, background, num_iter, num_moves, attempts, converged, draws —
 * whatever the other problems of the batch and their order.  Only `seconds` differs. */
int mcsas_hip_plan_launch_batch(mcsas_plan *const *plans, int32_t n, void *hip_stream);
int mcsas_hip_analyse_batch(const mcsas_problem *problems, int32_t n, mcsas_result *results);

/* ---- chains started from given contributions (ABI 5, additive): continue a run that ended at maxIterations, refine a result to
 * a tighter criterion, warm-start a frame of a series from an earlier frame's result -------------------------------------------
 * `start` is [n_contrib][n_active][rep_stride] in the layout of mcsas_result.contribs, so a fetched result feeds straight back;
 * repetition r of the plan reads column rep_first + r (0 <= rep_first, rep_first + n_reps <= rep_stride, else MCSAS_EINVAL).
 * The values are taken as they are and reach the model through the same clipping into the valueRange as any parameter set; they
 * need not lie inside gen_lo..gen_hi (a warm start under a narrowed active range is legal).  A non-finite value: MCSAS_EINVAL,
 * its index in mcsas_hip_last_error().
 * Contract: the FIRST attempt of each repetition is McSAS.mcFit with rset given in place of generateParameters(numContribs)
 *   (mcsas.py:317).  It consumes no uniforms for the initial set, so the step draws of that attempt start at index 0 of the chain's
 *   stream, replayed or Philox.  start_from_minimum is overridden for that attempt only.  num_iter counts from 0 and max_iter is
 *   the budget of THIS call.  Attempts after the first (the retry loop of analyse, mcsas.py:220-246) generate a fresh set exactly
 *   as they do without a start, draws included.  A start whose chi-squared already meets conv_crit returns itself: num_iter =
 *   num_moves = draws = 0, attempts = 1, converged = 1, contribs bit-equal to start.
 * mcsas_hip_plan_set_start: the plan keeps a (transposed) device copy taken at the call; the caller's array may be freed.  Every
 *   later launch of any slot, mcsas_hip_plan_launch_batch included, copies that block into the slot's parameter sets on the launch
 *   stream ahead of the kernel and runs the start form of the plan's kernel.  start == NULL clears it.  A batch groups plans by
 *   (model, q slots per lane, row cache, start or not): plans with and without a start may share one batch.
 *   mcsas_hip_plan_reseed and the replay stream are independent of the start.  A plan that resolved to MCSAS_EXEC_WAVE takes a
 *   start, and so does one that resolved to the q-split workgroup kernel (MCSAS_EXEC_WORKGROUP with more than 1024 q-points; not
 *   in a batch, which takes WAVE plans only); any other: MCSAS_EINVAL naming the mode (the plan stays usable).
 * mcsas_hip_analyse_from: mcsas_hip_analyse from `start` ([n_contrib][n_active][n_reps]).  MCSAS_EXEC_AUTO means WAVE, as in
 *   mcsas_hip_analyse_batch, whatever nq is: with AUTO or WAVE nq > 4096 is refused.  MCSAS_EXEC_WORKGROUP takes a start for
 *   1025...16384 q-points (the q-split kernel, the only one beyond 4096) and is refused up to 1024 (the workgroup-window kernel);
 *   PIPELINE is refused.  Every refusal comes before a device is touched, and so do those of a NULL start and a non-finite
 *   value.  n_active == 0 is answered as mcsas_hip_analyse answers it (start is not read).  n_devices > 1 shards as
 *   mcsas_hip_analyse does, each block reading its own columns of the one array.
 * Out of scope: mcsas_hip_analyse_host_rows (models that exist only as host code), the workgroup-window kernel (MCSAS_EXEC_WORKGROUP
 *   up to 1024 q-points) and the pipeline. */
int mcsas_hip_plan_set_start(mcsas_plan *plan, const double *start, int32_t rep_stride, int32_t rep_first);
int mcsas_hip_analyse_from(const mcsas_problem *problem, const double *start, mcsas_result *result);

/* ---- the accepted moves of a chain (ABI 5, additive): what the reference prints while mcFit runs ("good iter ...: Chisqr= ...",
 * mcsas.py:385-390), so that a caller sees whether a fit was still improving, had stalled or was cut off by maxIterations ---------
 * One wavefront per chain (MCSAS_EXEC_WAVE), or the q-split workgroup kernel (MCSAS_EXEC_WORKGROUP with 1025...16384 q-points:
 * the only kernel beyond 4096), cold or started (the start functions above).  Per repetition the trace holds the moves of its
 * LAST attempt, because num_iter and num_moves are that attempt's too: a retry (mcsas.py:220-246) starts it again.
 * Records kept: the first min(count, capacity) moves, in order; entries from there on are step = -1, chisq = NaN, values = NaN.
 *   count is always the full number of moves (== mcsas_result.num_moves), whatever the capacity.
 * The trace only observes: with a trace set, every array of mcsas_result except `seconds` is bit for bit that of the same call
 *   without one (mcsas_hip_analyse in the same mode, or with a start the from-form of it); start, the reseed call, the replay
 *   stream and `stop` behave as they do without a trace.  Cost: one bounds test and 2 + n_active stores per ACCEPTED move,
 *   nothing in a rejected step.  Measured once (one MI355X, Sphere 512 q x 400 contributions x 256 repetitions x 20000 steps,
 *   1205 moves per chain, capacity 4096): 26.87 ms of kernel against 26.50 ms untraced, +1.4 %, where two untraced runs differed
 *   by 0.004 ms (profiles/r17_summary.md) — small, but more than the noise: leave the trace off where it is not read.  The
 *   q-split kernel (thread 0 of the workgroup writes; Sphere 2048 q x 300 contributions x 256 repetitions x 20000 steps, capacity
 *   4096): 45.13 ms of kernel against 46.26 ms untraced, a ratio of 0.975 — the traced kernel was 2.5 % FASTER, where two
 *   untraced runs differed by 0.22 ms; more than the noise, cause not established (profiles/r19_summary.md): there a trace costs
 *   nothing measurable.
 * mcsas_hip_plan_set_trace: for a plan that resolved to MCSAS_EXEC_WAVE or to the q-split kernel (MCSAS_EXEC_WORKGROUP with more
 *   than 1024 q-points); any other: MCSAS_EINVAL naming the mode (the plan stays usable).  Every later launch of either slot runs
 *   the traced form of the plan's kernel, cold or started, and each slot owns its trace buffers.  capacity >= 1 and n_reps *
 *   capacity * (16 + 8 n_active) bytes <= 2 GiB, else MCSAS_EINVAL; capacity 0 clears. mcsas_hip_plan_launch_batch refuses a plan
 *   with a trace (MCSAS_EINVAL, nothing is launched).
 * mcsas_hip_plan_fetch_trace: after the slot's result has been fetched.  MCSAS_EINVAL if the plan has no trace, if
 *   trace->capacity differs from the plan's, on a NULL array or a wrong struct_size, or if the slot's launch was not traced.
 * mcsas_hip_analyse_traced: the one-shot form; `start` as for the from-form above, or NULL for a cold run.  MCSAS_EXEC_AUTO means
 *   WAVE, as it does for a start: with AUTO or WAVE nq > 4096 is refused, and the message names MCSAS_EXEC_WORKGROUP, which keeps
 *   a trace for 1025...16384 q-points.  WORKGROUP up to 1024 q-points, PIPELINE and n_devices > 1 are refused, and so are a NULL
 *   trace, a NULL array in it, capacity < 1, a wrong struct_size and a non-finite start value — every refusal before a device is
 *   touched.  n_active == 0 is answered as mcsas_hip_analyse answers it, with count[0] = 0.
 * Out of scope (each refuses): batches, device lists, the workgroup-window and pipeline kernels, mcsas_hip_analyse_host_rows. */
typedef struct mcsas_trace {
    uint32_t struct_size;  /* sizeof(mcsas_trace) */
    int32_t  capacity;     /* records kept per repetition */
    int64_t *count;        /* [n_reps] accepted moves of the last attempt (== mcsas_result.num_moves) */
    double  *chisq0;       /* [n_reps] reduced chi-squared of that attempt's initial set (mcsas.py:343-344) */
    int64_t *step;         /* [capacity][n_reps] numIter at which move i was accepted (0-based; contribution = step % n_contrib) */
    double  *chisq;        /* [capacity][n_reps] conval after the move: the number the chain compares with conv_crit (mcsas.py:379) */
    double  *values;       /* [capacity][n_active][n_reps] the accepted parameter set rt, as written to rset (mcsas.py:381) */
} mcsas_trace;
int mcsas_hip_plan_set_trace(mcsas_plan *plan, int32_t capacity);
int mcsas_hip_plan_fetch_trace(mcsas_plan *plan, int32_t slot, mcsas_trace *trace);
int mcsas_hip_analyse_traced(const mcsas_problem *problem, const double *start, mcsas_result *result, mcsas_trace *trace);

/* ---- one population fitted to several data sets: a scale per set or one for all, a background per set (ABI 5, additive) ---------
 * The same specimen measured more than once (two detector distances, SAXS + WAXS, two instruments): curves that overlap in q,
 * whose relative scale is not known well enough to merge them and whose backgrounds differ.  mcFit (mcsas.py:354-404) and
 * BackgroundScalingFit.calc (backgroundscalingfit.py:112-139) know one curve; this call extends them.  A chain holds ONE set of
 * n_contrib contributions; a row (calcIntensity) is evaluated at the q-points of all n_sets sets with the model's one parameter
 * vector.  At every fit — initial, per step, final — each set s gets the closed-form least-squares scale (and, with
 * find_background, background) of its own points, and the chain minimises the reduced chi-squared over ALL points:
 *   chi² nq = X = sum_s (S_s - num_s²/den_s),   a step is accepted iff X_t < X (strict, mcsas.py:379),
 * where S, num, den are SII, SIC, SCC of the set, centred (S = SII - SI²/Sw, num = SIC - SI SC/Sw, den = SCC - SC²/Sw) when a
 * background is fitted.  Convergence, retries and max_iter use chi² = X / nq as the single-set chain uses its chi².  Everything else
 * is mcsas_hip_analyse in MCSAS_EXEC_WAVE with cached rows: the draw order, the replay stream, Philox keyed by rep_offset + rep,
 * start_from_minimum, `stop`; with n_sets = 1 the chain takes that call's decisions.
 * problem->q / intensity / sigma hold the sets one after the other, set_nq[s] points each (>= 3), nq == sum set_nq.  One wavefront
 *   per chain: set s takes ceil(set_nq[s] / 64) register slots of 64 entries, and all sets together at most 16 slots.
 * result: as mcsas_hip_analyse; fit[nq][n_reps] holds every point with its own set's scale and background, chisq is the direct
 *   residual sum over all points / nq, scaling and background are set 0's.  sets (caller-allocated, arrays [n_sets][n_reps], an
 *   array left NULL is not written): each set's scale, background and sum over the set of ((I - fit) / sigma)² / set_nq[s].
 * Refused with MCSAS_EINVAL and a message that names the cause, before a device is touched: n_sets outside 1..MCSAS_MAX_SETS, a
 *   set of fewer than 3 points, sum set_nq != nq, more than 16 slots, positive_background, smearing (smear_nk > 0), a device list
 *   (n_devices > 1), a model plug-in or a model that exists only as host code, n_active == 0, cache_intensities == 0, an exec_mode
 *   other than MCSAS_EXEC_AUTO or MCSAS_EXEC_WAVE, a wrong struct_size.  There is no plan, slot, batch, start or trace form.
 * Scale mode (mcsas_hip_analyse_sets_mode; mcsas_hip_analyse_sets is the call with MCSAS_SETS_SCALE_PER_SET):
 *   MCSAS_SETS_SCALE_PER_SET  every set has a scale of its own, as above: curves whose relative scale is not known.
 *   MCSAS_SETS_SCALE_SHARED   curves on an absolute scale: ONE scale A for all sets, a background per set — the closed form of the
 *     (1 + n_sets)-unknown least-squares problem from the same per-set sums: with S_s, num_s, den_s as above,
 *       X_t = sum_s S_s - (sum_s num_s)² / (sum_s den_s),   accepted iff X_t < X,
 *     the three sums taken in set order; at the initial and final fit A = sum num_s / sum den_s, b_s = (SI_s - A SC_s) / Sw_s (0
 *     without find_background) and X is the sum of the sets' residual sums at (A, b_s).  sets->scaling[s] is A for every s,
 *     backgrounds and chisq are per set, result->scaling / background are A and b_0.  With n_sets = 1 the two modes are the same
 *     chain bit for bit.  A known relative scale k_s between the curves is the caller's: divide that set's intensity and sigma by it.
 *   An unknown mode is refused with MCSAS_EINVAL.
 * Not offered: fixed model parameters per set (contrast variation). */
#define MCSAS_SETS_SCALE_PER_SET 0
#define MCSAS_SETS_SCALE_SHARED  1
#define MCSAS_MAX_SETS 4
typedef struct mcsas_sets_result {
    uint32_t struct_size;  /* sizeof(mcsas_sets_result) */
    int32_t  n_sets;       /* rows of the arrays below: the call's n_sets */
    double  *scaling;      /* [n_sets][n_reps] */
    double  *background;   /* [n_sets][n_reps] */
    double  *chisq;        /* [n_sets][n_reps] sum over the set / set_nq[s] */
} mcsas_sets_result;
int mcsas_hip_analyse_sets(const mcsas_problem *problem, int32_t n_sets, const int32_t *set_nq,
                           mcsas_result *result, mcsas_sets_result *sets);
int mcsas_hip_analyse_sets_mode(const mcsas_problem *problem, int32_t n_sets, const int32_t *set_nq, int32_t scale_mode,
                                mcsas_result *result, mcsas_sets_result *sets);

/* ---- McSAS.histogram() of a joint fit: the sets of mcsas_hip_analyse_sets seen together (ABI 5, additive) -------------------------
 * mcsas_hip_histogram where problem->q / intensity / sigma hold n_sets sets one after the other, unpadded, set_nq[s] points each
 * (>= 3, nq == sum set_nq).  Per repetition: the rows and their sum over all nq points as there; then
 *   the fit: MCSAS_SETS_SCALE_PER_SET the closed-form scale and background of each set on its own points (the sums as
 *     mcsas_hip_histogram forms them for one curve), MCSAS_SETS_SCALE_SHARED the one scale and per-set backgrounds of
 *     mcsas_hip_analyse_sets_mode; A_ref is the scale of set ref_set (the shared scale in shared mode);
 *   the visibility limit of a contribution: with vf = w A_ref / v, the minimum over the points k of the sets named in visible_sets
 *     (bit s: set s) of (sigma[k] vf) / (A_s(k) row[k]), points whose A_s(k) row[k] is zero left out, +inf where none is kept;
 *   fractions, bins, cumulative distribution and moments: as mcsas_hip_histogram with A_ref.
 * scaling[2][n_reps] = (A_ref, b of ref_set); sets (arrays [n_sets][n_reps], caller-allocated): every set's scale and background;
 *   sets->chisq may be NULL and is not written.  fractions, out, specs: as mcsas_hip_histogram.  With n_sets == 1 every number is
 *   mcsas_hip_histogram's bit for bit; in per-set mode with visible_sets == 1 << ref_set the scaling, fractions and histograms are
 *   those of mcsas_hip_histogram on that set alone.
 * Refused with MCSAS_EINVAL and a message that names the cause, before a device is touched: whatever mcsas_hip_histogram refuses,
 *   n_sets outside 1..MCSAS_MAX_SETS, sum set_nq != nq, a set of fewer than 3 points, ref_set outside the sets, visible_sets empty
 *   or naming a set that is not there, an unknown scale_mode, positive_background, smearing, a model plug-in or a host model.
 * The call takes no partial-intensity wishes (`want`) and has no batch and no device-rows form; 2-D histograms are made from the
 *   fractions (mcsas_hip_histogram2d) and need nothing of their own. */
struct mcsas_histogram_spec;   /* (defined with mcsas_hip_histogram, further down) */
int mcsas_hip_histogram_sets(const mcsas_problem *problem, const double *contribs, int32_t n_hist, const struct mcsas_histogram_spec *specs,
                             int32_t n_sets, const int32_t *set_nq, int32_t scale_mode, int32_t ref_set, uint32_t visible_sets,
                             double *scaling, double *fractions, double *out, mcsas_sets_result *sets);

/* ---- ScatteringModel.calc(data, pset, compensationExponent) (scatteringmodel.py:79-109) ------
 * Uses problem->{model_id, params, n_active, active_index, clip_*, nq, q, comp_exp, device}.
 * pset[n][n_active] -> cum_int[nq] (rows summed in order), vset/wset/sset[n], optional
 * rows[n][nq] (each contribution's F²·w, i.e. SASModel.calcIntensity()[0], sasmodel.py:46-79). */
int mcsas_hip_model_calc(const mcsas_problem *problem, const double *pset, int32_t n,
                         double *cum_int, double *vset, double *wset, double *sset, double *rows);

/* ---- BackgroundScalingFit.calc (backgroundscalingfit.py:112-139), closed-form minimiser ------
 * out[4] = { sc[0] (scaling), sc[1] (background), conval (reduced chi²), aGoFs } */
int mcsas_hip_bgfit(int32_t nq, const double *intensity, const double *sigma, const double *model_int,
                    int32_t find_background, int32_t positive_background, int32_t num_params,
                    int32_t device, double out[4]);

/* ---- McSAS.histogram()'s per-contribution visibility limits (mcsas.py:575-594) --------------
 * For each rep: min over q of sigma·vf_c / (A·I_c(q)) where I_c != 0.  contribs in the
 * (n_contrib, n_active, n_reps) layout of mcsas_result, vol_frac/min_req_vol [n_contrib][n_reps]. */
int mcsas_hip_observability(const mcsas_problem *problem, const double *contribs,
                            const double *scaling, const double *vol_frac, double *min_req_vol);

/* ---- McSAS.histogram(), first half, for ALL repetitions in one call (mcsas.py:549-594) ----------
 * Per rep: model.calc over its contributions (:552), scale/background fit of the summed intensity to
 * the data (:559), per-contribution visibility limits min_q sigma*vf_c / (A*I_c(q)) (:575-590) with
 * vf_c = wset_c * A / vset_c (modeldata.py:57-61).  Uses problem->{model, nq, q, intensity, sigma,
 * n_contrib, n_reps, comp_exp, find_background, positive_background, smear_*, device}; contribs in the
 * (n_contrib, n_active, n_reps) layout of mcsas_result.  scaling[2][n_reps] = (A, b) per rep;
 * vset/wset/sset/min_req_vol [n_contrib][n_reps]. */
int mcsas_hip_histogram_prep(const mcsas_problem *problem, const double *contribs, double *scaling,
                             double *vset, double *wset, double *sset, double *min_req_vol);

/* ---- McSAS.histogram(), ALL of it for all repetitions in one call (mcsas.py:445-615) --------------
 * What mcsas_hip_histogram_prep does, then on the device as well: the volume / number / intensity / surface fractions and
 * their visibility limits with the per-repetition normalisation (mcsas.py:561-604), and for every configured histogram
 * (utils/parameter.py:187-538: one per (parameter, range, weighting)) the bins, the mean visibility limit of a bin's
 * members, the cumulative distribution (Histogram._calcBins / _calcCDF :441-479) and the moments per repetition
 * (Moments :84-122) — every sum taken over the contributions in contribution order, the order of the reference's
 * builtin sum().  The means / standard deviations over the repetitions (VectorResult :156-184) are left to the caller.
 *   specs[h]: param_index = column of contribs; weighting 0 vol, 1 num, 2 int, 3 surf; edges = n_bin + 1 lower bin edges
 *             (Histogram._setXLowerEdge :349-362, evaluated by the caller so that bin membership is numpy's); lower / upper =
 *             the histogram's value range (Moments count lower < x < upper).
 *   scaling[2][n_reps]; fractions[8][n_contrib][n_reps] = vol, num, int, surf fractions, then their visibility limits
 *   (may be NULL); out = per histogram, one after the other: bins[n_bin][n_reps], obs[n_bin][n_reps] (0 for an empty bin),
 *   cdf[n_bin][n_reps], moments[5][n_reps] (total, mean, variance, skew, kurtosis).
 * n_contrib <= 4096 (the contributions of a repetition are staged in LDS): MCSAS_EINVAL beyond, use mcsas_hip_histogram_prep. */
typedef struct mcsas_histogram_spec {
    int32_t param_index, weighting, n_bin, reserved;
    double  lower, upper;
    const double *edges;
} mcsas_histogram_spec;
int mcsas_hip_histogram(const mcsas_problem *problem, const double *contribs, int32_t n_hist,
                        const mcsas_histogram_spec *specs, double *scaling, double *fractions, double *out);

/* ---- McSAS.histogram() of a series: n_sets data sets in one call --------------------------------------------------------------
 * Set s means exactly mcsas_hip_histogram(&problems[s], contribs[s], n_hist[s], specs[s], scaling[s], fractions[s], out[s]) — the
 * same layouts, fractions[s] (or the table `fractions`) may be NULL — and every array of every set is that single call's bit for
 * bit, whatever else is in the batch and in whatever order.  What it saves is the calls: ONE packed upload, ONE launch per kernel
 * over the (set, repetition) blocks of all sets (the model's rows: one launch per built-in model present) and ONE packed download.
 *   e.g. a series' histograms after mcsas_hip_analyse_batch: mcsas_hip_histogram_batch(n, problems, contribs, n_hist, specs, sc, fr, out);
 * Refused with MCSAS_EINVAL before a device is touched, the message naming the set (and the histogram): n_sets < 0, a NULL table,
 * whatever mcsas_hip_histogram refuses of a set (n_contrib > 4096 among it), sets that name different devices.  n_sets == 0: MCSAS_OK.
 * Memory: the sets are taken in order, in chunks whose rows (n_contrib * n_reps * nq doubles per set) fit 2 GiB, or
 * MCSAS_HIP_HIST_BATCH_MB MiB (environment, read at every call, fractions allowed); the kernels run once per chunk.  A set whose
 * rows alone exceed that, and a set of a plug-in model (the run-time compiler has no batch form of its rows kernel), runs in its
 * place through mcsas_hip_histogram. */
int mcsas_hip_histogram_batch(int32_t n_sets, const mcsas_problem *problems, const double *const *contribs,
                              const int32_t *n_hist, const mcsas_histogram_spec *const *specs,
                              double *const *scaling, double *const *fractions, double *const *out);

/* ---- McSAS.histogram() of a model whose rows the caller computes ON THE DEVICE (additive to ABI 5) ------------------------------
 * mcsas_hip_histogram for the models of mcsas_hip_analyse_device_rows: contribs, n_hist, specs, scaling, fractions, out and the limit
 * n_contrib <= 4096 mean what they mean there, the layouts are the same; only the rows and the per-row volume / weight / surface come
 * from the caller's device code, a round at a time, and never cross the bus: one packed upload, per round the kernels, one packed
 * download.  A round is a block of whole repetitions [r0, r0 + k), k = min(n_reps - r0, capacity_rows / n_contrib) (65535 at the most);
 * row rl * n_contrib + c of the round is contribution c of repetition r0 + rl.
 *   d_pset [capacity_rows][n_active], d_rows [capacity_rows][row_stride], d_vws [3][capacity_rows]: the CALLER's device memory on
 *     problem->device; row_stride = nq (dense: ask mcsas_hip_histogram_rows_shape, never hard-code it).
 *   rows_cb(user, n): d_pset[0..n) holds the round's parameter sets (activeParams() order, NOT clipped, taken from contribs[c][p][r]),
 *     complete on the device when the callback is entered; the callback fills columns 0..nq of rows 0..n of d_rows and entries 0..n
 *     of each third of d_vws (volume, weight, surface of each row, the order calcIntensity returns them), complete on the device when
 *     it returns; return 0, anything else aborts with MCSAS_ECALLBACK.  Calling thread only, between the library's launches.
 *   mcsas_hip_histogram_rows_shape (touches no device): *min_rows = n_contrib is the least capacity_rows (one repetition per round);
 *     *useful_rows = n_contrib * n_reps, capped by 256 MiB / (row_stride * 8) rounded down to whole repetitions, never below
 *     min_rows; *row_stride as above.  Any of the three may be NULL.
 * Uses problem->{nq, q, intensity, sigma, n_active, n_contrib, n_reps, find_background, positive_background, device}; model_id,
 * params, clip_*, comp_exp are the callback's business.  Smearing is not: a problem that carries a smearing table is refused.
 * Refused with MCSAS_EINVAL before a device is touched: NULL problem / contribs / d_pset / d_rows / d_vws / rows_cb / out, a wrong
 * struct_size, capacity_rows < n_contrib, a smearing table, and whatever mcsas_hip_histogram refuses of sizes and histogram records
 * (the same sentences behind "histogram_device_rows: "); after the device is selected, before anything is launched: a buffer that is
 * not device memory of that device (MCSAS_EINVAL).  A failed allocation of the staging blocks: MCSAS_ENOMEM.
 * Fed the rows of a built-in model, every array is mcsas_hip_histogram's bit for bit, whatever the rounds (tests/test_hist_rows_gpu.py). */
int mcsas_hip_histogram_rows_shape(const mcsas_problem *problem, int64_t *min_rows, int64_t *useful_rows, int32_t *row_stride);
int mcsas_hip_histogram_device_rows(const mcsas_problem *problem, const double *contribs,
                                    double *d_pset, double *d_rows, double *d_vws, int64_t capacity_rows,
                                    mcsas_device_rows_callback rows_cb, void *user,
                                    int32_t n_hist, const mcsas_histogram_spec *specs,
                                    double *scaling, double *fractions, double *out);

/* ---- the partial intensities of histogram ranges and bins (additive to ABI 5; Moments.intensity, utils/parameter.py:124-154) -----
 * mcsas_hip_histogram, and mcsas_hip_histogram_device_rows, with one more result: the scattering curve of only the contributions
 * inside a histogram's value range, and of each of its bins, scaled by the repetition's fitted scale A = scaling[0][r] — taken on
 * the device from the rows the call has in HBM anyway, before they are thrown away.  No row crosses the bus, no form factor is
 * evaluated twice.  With rows[c][k] the (smeared, where the call smears) intensity row of contribution c and x_c = contribs[c][p][r]:
 *   range[k][r]  = A * sum_c rows[c][k] over lower < x_c < upper, both strict (the mask of the moments); no background is added
 *   bin[b][k][r] = A * sum_c rows[c][k] over edges[b] <= x_c < edges[b+1] && x_c < edges[n_bin] (the members of bin b)
 * Each sum runs in contribution order from +0.0 and is multiplied by A ONCE, at the end: an IEEE ordered sum and one product, which
 * numpy reproduces bit for bit (mcsas_amd/parameter.py: partial_intensities).  An empty selection gives A * 0.0; a NaN parameter
 * value is in no bin and in no range; NaN or inf in a row propagate by IEEE's rules.
 *   want[h]: 0 nothing, 1 the range curve, 2 the range curve and the bin curves of histogram h.
 *   partial = for each histogram with want >= 1, in order: range[nq][n_reps], then, if 2, bin[n_bin][nq][n_reps].
 * scaling, fractions and out are what the call without `want` returns for the same arguments, bit for bit; with every want 0 (or
 * n_hist == 0) the call IS that call and partial is not looked at.
 * Refused with MCSAS_EINVAL before a device is touched, after whatever the plain call refuses (its sentences unchanged), each
 * message behind "histogram_partial: " and naming the histogram: want NULL with n_hist > 0; a want outside 0..2; partial NULL while
 * something is wanted; want 2 with n_bin > 256 (a bin's running sums lie in LDS: 256 * 64 doubles; the range curve has no such
 * cap); want 2 with edges that are not finite and non-decreasing (a contribution is filed under ONE bin; want <= 1 keeps the plain
 * call's permissiveness); curves of more than 2 GiB in all.  mcsas_hip_histogram_batch has no partial form. */
int mcsas_hip_histogram_partial(const mcsas_problem *problem, const double *contribs, int32_t n_hist,
                                const mcsas_histogram_spec *specs, const int32_t *want,
                                double *scaling, double *fractions, double *out, double *partial);
/* The same for rows the caller computes on the device: mcsas_hip_histogram_device_rows' arguments, then want and partial as above.
 * The curves of a round are taken from d_rows as the callback left them, before the next round overwrites them. */
int mcsas_hip_histogram_partial_device_rows(const mcsas_problem *problem, const double *contribs,
                                            double *d_pset, double *d_rows, double *d_vws, int64_t capacity_rows,
                                            mcsas_device_rows_callback rows_cb, void *user,
                                            int32_t n_hist, const mcsas_histogram_spec *specs, const int32_t *want,
                                            double *scaling, double *fractions, double *out, double *partial);

/* ---- the joint histogram of TWO fit parameters (additive to ABI 5; the reference has no counterpart) ----------------------------
 * Takes the fractions a histogram call returned and evaluates no model: it serves every path that ends in them, and doubles of the
 * caller's own.  contribs [n_contrib][n_active][n_reps] as in mcsas_result; fractions [8][n_contrib][n_reps] as mcsas_hip_histogram
 * returns them (vol, num, int, surf fractions, then their visibility limits).
 *   specs[h]: param_x / param_y = columns of contribs (they may be equal); weighting 0 vol, 1 num, 2 int, 3 surf; edges_x / edges_y =
 *             n_bin_x + 1 / n_bin_y + 1 lower edges, finite and non-decreasing (equal neighbours: an empty column); lower_* / upper_*
 *             = the value ranges of the moments; reserved must be 0.  An axis without bins does not read its edges.
 *   out = per histogram, one after the other: bins[n_bin_x][n_bin_y][n_reps], obs[n_bin_x][n_bin_y][n_reps], moments[7][n_reps]
 *         (total, mean x, mean y, variance x, variance y, covariance, correlation).
 * Per axis the rules are the 1-D call's.  With edges e[0..n] a value x lies in column i = #{k : e[k] <= x} - 1 iff 0 <= i < n (a NaN
 * in none); a contribution is in cell (i, j) iff it is in column i of x and column j of y.  bins = the sum of the weighting's fraction
 * over the cell's members in contribution order (a NaN sum is stored as 0), obs = the same sum of their visibility limits over their
 * count (0 for an empty cell).  The moments run over the contributions with lower_x < x < upper_x && lower_y < y < upper_y, every sum
 * in contribution order: tot = S f; mx = S x f (/ tot unless tot == 0), my alike; vxx = S ((dx dx) f) / tot with dx = x - mx, vyy
 * alike; cxy = S ((dx dy) f) / tot; rho = cxy / (sqrt|vxx| sqrt|vyy|) unless that product is exactly 0 (then 0; NaN goes on);
 * all seven 0 where no contribution is inside.  With a y range that holds every value tot, mx, vxx are the 1-D call's total, mean,
 * variance bit for bit, and with one y column that holds every value bins and obs are the 1-D call's.
 * 1 <= n_contrib <= 4096, n_bin_x, n_bin_y >= 0 with n_bin_x * n_bin_y <= 4096 (zero bins on an axis: moments only).
 * Refused with MCSAS_EINVAL before a device is touched, the message naming the histogram: NULL tables, n_hist < 0, a non-zero
 * reserved, sizes and indices outside those limits, edges that are not finite or fall.  n_hist == 0: MCSAS_OK, no device touched. */
typedef struct mcsas_histogram2d_spec {
    int32_t param_x, param_y, weighting, n_bin_x, n_bin_y, reserved;
    double  lower_x, upper_x, lower_y, upper_y;
    const double *edges_x, *edges_y;
} mcsas_histogram2d_spec;
int mcsas_hip_histogram2d(int32_t n_contrib, int32_t n_active, int32_t n_reps, const double *contribs, const double *fractions,
                          int32_t n_hist, const mcsas_histogram2d_spec *specs, double *out, int32_t device);

/* ---- input preparation ----------------------------------------------------------
 * DataObj._prepareUncertainty (dataobj/dataobj.py:204-227): sigma_out = max(sigma_raw, fu_min * I),
 * fu_min * I when sigma_raw is NULL (no uncertainty column), +inf where that is not finite. */
int mcsas_hip_prepare_uncertainty(int32_t n, const double *intensity, const double *sigma_raw, double fu_min,
                                  int32_t device, double *sigma_out);
/* DataObj._reBin (dataobj/dataobj.py:288-345) on the sanitized vectors x, f, fu [n]: bin b takes the
 * points with edges[b] <= x < edges[b+1] (edges[n_bin+1]: the caller's numpy.logspace, :312-316); one
 * point: copied; more: mean x, mean f, max(std(f, ddof=1)/sqrt(count), sqrt(sum fu^2 / count)); empty
 * bins are dropped.  Outputs hold up to n_bin entries, *n_out = bins kept. */
int mcsas_hip_rebin(int32_t n, const double *x, const double *f, const double *fu, int32_t n_bin,
                    const double *edges, int32_t device, double *x_out, double *f_out, double *fu_out,
                    int32_t *n_out);

/* Run-time model plug-in — what the reference's model discovery does for any file under models/ with a ScatteringModel subclass
 * (utils/findmodels.py:120-186; the four methods a model supplies: bases/model/scatteringmodel.py:15-58, sasmodel.py:36-79).
 * `source` is HIP C++ text that defines, per q point and on the model's full parameter vector p[MCSAS_MAX_PARAMS] (active
 * parameters substituted and clipped into their valueRange):
 *     __device__ double mcsas_plugin_formfactor(double q, const double *p);   // ScatteringModel.formfactor
 *     __device__ double mcsas_plugin_volume(const double *p);                  // .volume()
 *     __device__ double mcsas_plugin_absvolume(const double *p);               // .absVolume()
 *     __device__ double mcsas_plugin_surface(const double *p);                 // .surface()
 * (csrc/fastmath.h and device_util.h are in scope, namespace mcsas.)  The text is compiled with hiprtc for gfx950 against
 * the library's own kernel headers, which it carries inside; no GPU is needed for that.  *model_id (>= MCSAS_MODEL_PLUGIN0)
 * is then valid as mcsas_problem.model_id in every entry point and every execution mode (the chain kernel of the mode is
 * compiled for the plug-in on first use: 0.5 - 15 s once per q-slot count; more than 1024 q-points: the q-split workgroup
 * kernel, MCSAS_EXEC_AUTO or MCSAS_EXEC_WORKGROUP); beam-profile smearing if the text
 * says `#define MCSAS_PLUGIN_CAN_SMEAR 1` (the model class's canSmear).  A form
 * factor that loops over orientations / a contour should say `#define MCSAS_PLUGIN_ROW_CLASS 1` (csrc/plugin_model.h: how
 * the pipeline spreads such rows over the chip; results do not depend on it).  The same text registered twice
 * gives the same id.  MCSAS_EINVAL + mcsas_hip_plugin_log() (compiler output, calling thread) if it does not compile. */
int         mcsas_hip_plugin_compile(const char *source, int32_t *model_id);
const char *mcsas_hip_plugin_log(void);

/* A (non-blocking) HIP stream on `device` for mcsas_hip_plan_launch, for hosts that have no HIP binding of their own: plans on
 * different streams overlap on the chip — two analyses side by side finish sooner than one after the other. */
int         mcsas_hip_stream_create(int32_t device, void **stream);
void        mcsas_hip_stream_destroy(void *stream);
/* Device and pinned memory that destroyed plans gave back stays parked for the next plan of the same shape (a series of
 * analyses pays ~3 ms per plan in hipFree / hipHostFree otherwise), up to 4 GiB per process; this returns it to the driver. */
int         mcsas_hip_release_cached_memory(void);
int         mcsas_hip_device_count(void);
int         mcsas_hip_abi_version(void);
/* 0: the release library.  1: a measurement build (-DMCSAS_TUNING) in which mcsas_problem.reserved0 selects tuning and
 * ablation variants of the pipeline mode (csrc/mcsas_hip.hip, mcsas_hip_plan_create); never shipped as libmcsas_hip.so */
int         mcsas_hip_is_tuning_build(void);
const char *mcsas_hip_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* MCSAS_HIP_H */
