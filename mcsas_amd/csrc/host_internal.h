// host_internal.h — what the host units of libmcsas_hip.so share (mcsas_hip.hip: plans, the memory cache, the stop word; host_decide.hip: what is decided without a
// device, the chain settings and the weights among it; host_analyse.hip: one-shot analyses; host_rows.hip: rows evaluated by the caller; host_plugin.hip: run-time compiler of
// model plug-ins; host_calls.hip: small one-call entry points; host_hist.hip: McSAS.histogram(); host_sets.hip: the device half of one population fitted to several data sets;
// small_launch.h: from a model id to a small kernel's instance, for host_calls.hip and host_hist.hip).  Host code only: the run-time compiler never sees this file (it is not among the embedded headers).
#pragma once
#include <hip/hip_runtime.h>
#include <new>
#include <string>
#include <vector>

#include "../../include/mcsas_hip.h"
#include "chain_common.h"

#pragma GCC visibility push(hidden)

// ------------------------------------------------------------------------------ error plumbing (host_decide.hip)
extern thread_local std::string g_err;
int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
// an inner check's refusal passed on in the caller's name: "<fmt and its arguments>: <what g_err said>", the code kept
int fail_within(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
#define HIPCHK(expr)                                                                         \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess)                                                                \
            return fail(e_ == hipErrorOutOfMemory ? MCSAS_ENOMEM : MCSAS_EHIP, "%s: %s (%s:%d)", \
                        #expr, hipGetErrorString(e_), __FILE__, __LINE__);                   \
    } while (0)

// the C boundary of the one-shot chain calls (host_rows.hip, host_sets.hip): a host vector that cannot be had is MCSAS_ENOMEM, no exception
template <class F> int no_bad_alloc(const char *who, F f) {
    try { return f(); } catch (const std::bad_alloc &) { return fail(MCSAS_ENOMEM, "%s: out of host memory", who); }
}

int select_device(int device);
// A buffer the caller hands over as device memory (host_rows.hip; mcsas_hip_analyse_device_rows, mcsas_hip_histogram_device_rows):
// MCSAS_EINVAL in `who`'s name unless `ptr` is unmanaged device memory of device `dev`.  Asked before a kernel is launched on it.
int check_device_buffer(const char *who, const char *name, const void *ptr, int dev);

// Every entry point that selects a device puts the calling thread's current device back on the way out: a
// host that shares the HIP runtime (torch with RCCL in bench.py, the hosts of INTEGRATION.md) keeps its own.
struct DeviceGuard {
    int prev = -1;
    DeviceGuard() { if (hipGetDevice(&prev) != hipSuccess) prev = -1; }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
    DeviceGuard(const DeviceGuard &) = delete;
    DeviceGuard &operator=(const DeviceGuard &) = delete;
};

// ------------------------------------------------------------------------------ the process-level memory cache (mcsas_hip.hip: MemCache)
hipError_t cached_dev_malloc(void **p, size_t n);
void cached_dev_free(void *p, size_t n, int d);
hipError_t cached_host_malloc(void **p, size_t n, unsigned flags);
void cached_host_free(void *p, size_t n, unsigned flags);
hipError_t cached_copy_stream(hipStream_t *st);

// McSAS.stop as the kernels see it (chain_common.h: stop_requested): one pinned, mapped word from the cache, `d` its device address;
// back to the cache with its owner — a plan, a batch, a call of mcsas_hip_analyse_sets
struct StopWord {
    int32_t *h = nullptr, *d = nullptr;
    hipError_t make();                                     // *h = 0
    ~StopWord() { cached_host_free(h, sizeof(int32_t), hipHostMallocMapped); }
    StopWord() = default;
    StopWord(const StopWord &) = delete;
    StopWord &operator=(const StopWord &) = delete;
};
// Waits for `done`, forwarding the caller's stop word to the device-visible one every 50 us meanwhile (McSAS.stop, mcsas.py:357);
// no caller's word: nothing to forward, a plain wait.  An error of the event is "<who>kernel failed: ...".
int wait_forwarding_stop(const char *who, hipEvent_t done, const volatile int32_t *caller_stop, int32_t *h_stop);
// the caller's replay streams, [R][replay_len], to the device
inline hipError_t copy_replay(double *dst, const mcsas_problem *p, size_t R) {
    return hipMemcpy(dst, p->replay_stream, sizeof(double) * R * (size_t)p->replay_len, hipMemcpyHostToDevice);
}

// scratch arrays of the one-call entry points and of mcsas_hip_analyse_host_rows: from / back to the process-level cache (a
// histogram() makes a dozen of them)
template <typename T> struct DevBuf {
    T *p = nullptr;
    size_t bytes = 0;
    int dev = 0;
    ~DevBuf() {
        if (!p) return;
        (void)hipStreamSynchronize(nullptr);       // (hipFree used to wait for the kernels that read it — they run on the null stream —; the cache does not)
        cached_dev_free(p, bytes, dev);
    }
    hipError_t alloc(size_t n) {
        bytes = (sizeof(T) * (n ? n : 1) + 255) / 256 * 256;
        (void)hipGetDevice(&dev);
        return cached_dev_malloc((void **)&p, bytes);
    }
};

// ------------------------------------------------------------------------------ the chain kernel families
// A kernel is (family, given): the wave, wave-batch and q-split families have a second form whose first attempt takes a given set
// (mcsas_hip_plan_set_start), the workgroup-window and pipeline families have none.  Every built-in model has its instances in
// kern_*.hip (the started ones in kern_wave_start.hip and kern_wide_start.hip), a plug-in compiles its own on first use.  The traced
// families (kern_wave_trace.hip, kern_wide_trace.hip) also record their accepted moves (mcsas_hip_plan_set_trace), cold and started.
enum KernelFamily { KF_WAVE, KF_WAVE_BATCH, KF_WG, KF_WIDE, KF_PIPE_TICK, KF_WAVE_TRACE, KF_WIDE_TRACE, KF_COUNT };

// One row per family, the one place that says what a family is: the word for it in messages; the kernel template's name (namespace
// mcsas) and the key of a plug-in's program; whether the template has, behind <model, qpl>, a flag (the row cache of the wave families,
// rows pulled from a queue by the pipeline tick) and GIVEN; whether the kernel's last argument is the launch's TraceArgs; what it takes
// between its argument block and those (nothing, the WgGeom, q3inv); its block: one wave, the plan's waves per chain, PIPE_BLOCK threads.
struct FamilyInfo {
    const char *word, *kernel, *key;
    bool flagged, startable, trace;
    enum Arg2 { ARG2_NONE, ARG2_WG, ARG2_Q3INV } arg2;
    enum Block { BLOCK_WAVE, BLOCK_WAVES, BLOCK_PIPE } block;
};

constexpr FamilyInfo KERNEL_FAMILY[KF_COUNT] = {
    {"", "chain_wave_kernel", "wave", true, true, false, FamilyInfo::ARG2_NONE, FamilyInfo::BLOCK_WAVE},
    {"batch ", "chain_wave_batch_kernel", "wave batch", true, true, false, FamilyInfo::ARG2_NONE, FamilyInfo::BLOCK_WAVE},
    {"", "chain_wg_kernel", "wg", false, false, false, FamilyInfo::ARG2_WG, FamilyInfo::BLOCK_WAVES},
    {"q-split ", "chain_wide_kernel", "wide", false, true, false, FamilyInfo::ARG2_Q3INV, FamilyInfo::BLOCK_WAVES},
    {"pipeline ", "pipe_tick_kernel", "pipe", true, false, false, FamilyInfo::ARG2_NONE, FamilyInfo::BLOCK_PIPE},
    {"traced ", "chain_wave_trace_kernel", "wave trace", true, true, true, FamilyInfo::ARG2_NONE, FamilyInfo::BLOCK_WAVE},
    {"traced q-split ", "chain_wide_trace_kernel", "wide trace", false, true, true, FamilyInfo::ARG2_Q3INV, FamilyInfo::BLOCK_WAVES},
};

// ------------------------------------------------------------------------------ run-time model plug-ins (host_plugin.hip)
enum PluginSmallKernel { PLUGIN_MODEL_ROWS, PLUGIN_OBSERVABILITY, PLUGIN_HIST_ROWS };

inline bool is_plugin_model(int model_id) { return model_id >= MCSAS_MODEL_PLUGIN0 && model_id < MCSAS_MODEL_PLUGIN0 + MCSAS_MAX_PLUGINS; }
// what a plug-in's text declares (plugin_model.h); false: no such plug-in
bool plugin_declares(int model_id, int *row_class, bool *can_smear);
// the family's kernel for `qpl` q slots per lane, the family's flag (row cache / row queue; ignored by the families without one)
// and `given`, compiled on first use, as a function of the CURRENT device's module
int plugin_chain_function(int model_id, KernelFamily family, int qpl, bool flag, bool given, hipFunction_t *fn);
int plugin_small_function(int model_id, PluginSmallKernel which, hipFunction_t *fn);

// launch of a small kernel of a plug-in on the null stream; the arguments are passed by address, so their types must be the
// kernel's parameter types exactly — launch_small_kernel (small_launch.h) makes them so and is the only caller
template <class... A>
static int plugin_small_launch(int model_id, PluginSmallKernel which, dim3 grid, size_t lds, A... args) {
    hipFunction_t fn = nullptr;
    int rc = plugin_small_function(model_id, which, &fn);
    if (rc) return rc;
    void *ka[] = {(void *)&args...};
    HIPCHK(hipModuleLaunchKernel(fn, grid.x, grid.y, grid.z, mcsas::WAVE, 1, 1, (unsigned)lds, nullptr, ka, nullptr));
    return MCSAS_OK;
}

// ------------------------------------------------------------------------------ models (host_decide.hip)
// what the host needs to know about a model, read off its Contrib<M> (models.h) — no per-model code outside this table
struct ModelTraits { int int_div_param, rowtab, row_class; bool can_smear; int (*table_doubles)(int); int contrib_doubles; };
ModelTraits model_traits(int model_id);
inline int table_doubles_host(int model_id, int K) { return model_traits(model_id).table_doubles(K); }
// per-wave scratch for the per-row orientation table (Contrib<M>::ROWTAB * K doubles, models.h); beyond
// K = 256 the chain kernels evaluate the integrand directly
inline int rowtab_doubles_host(int model_id, int K) { return K > 256 ? 0 : model_traits(model_id).rowtab * K; }
int fill_model_args(const mcsas_problem *p, mcsas::ModelArgs *m);
// The weight rule, once: sigma == 0 -> 1 (backgroundscalingfit.py:117), w = 1 / e², wI = w I, and the sums over the n points in order,
// each first onto 0.0 (DESIGN §4.1e rests on these being the same IEEE operations for one set and for several)
struct WeighedSums { double Sw, SI, SII, Ssig2; };
WeighedSums weigh_points(const double *I, const double *sigma, int n, double *w, double *wI, double *Iout);

// Device copy of the smearing tables of a problem: locs transposed to [K][stride] (pad columns repeat
// column 0, like the padded q) and cw[m] = 2 * trapezoid coefficient(q_offset)[m] * weights[m], so that
// sum_m cw[m] y[m] = 2 trapz(y * weights, x = q_offset) (sasmodel.py:72-73).
struct SmearDev {
    double *locs_t = nullptr, *cw = nullptr;
    ~SmearDev() { if (locs_t) hipFree(locs_t); if (cw) hipFree(cw); }
    static bool active(const mcsas_problem *p);            // smearing asked for and the model can be smeared (canSmear)
    static int check(const mcsas_problem *p);              // the refusal of upload(), without a HIP call
    int upload(const mcsas_problem *p, int stride, mcsas::ModelArgs *m);
};

// ------------------------------------------------------------------------------ what a request is refused for, with and without a plan (host_decide.hip)
// plan_set_start / plan_set_trace / plan_fetch_trace and the one-shot entry points over them (host_analyse.hip) answer alike
// the first non-finite value of the columns [first, first + R) of start[N][P][stride], or MCSAS_OK
int check_start_finite(const char *who, const double *start, size_t N, size_t P, size_t stride, size_t first, size_t R);
int check_trace_arrays(const char *who, const mcsas_trace *tr);
const char *exec_mode_name(int mode);
// A slot's trace block: [step | chisq | values | chisq0] of R repetitions with room for K moves of P values each, on the host as
// fetched and in its 256-byte-aligned device block.  Step, chisq and values together stay below TRACE_MAX_BYTES.
constexpr size_t TRACE_MAX_BYTES = (size_t)2 << 30;
struct TraceLayout {
    size_t move_bytes, step, chisq, values, chisq0, host_bytes, dev_bytes;
    constexpr TraceLayout(size_t R, size_t K, size_t P)
        : move_bytes(16 + 8 * P), step(0), chisq(8 * R * K), values(16 * R * K), chisq0(move_bytes * R * K),
          host_bytes(chisq0 + 8 * R), dev_bytes((host_bytes + 255) / 256 * 256) {}
    static constexpr bool too_large(size_t R, size_t K, size_t P) { return K > TRACE_MAX_BYTES / (R * TraceLayout(R, 0, P).move_bytes); }
};

// ------------------------------------------------------------------------------ which kernel takes how many q-points, a start, a trace
// The q-points a kernel takes (host_decide.hip ties them to WAVE and WIDE_MAX_WAVES): the workgroup-window kernel and the pipeline, one
// wavefront per chain (32 / 64 q slots per lane beyond the first), the q-split kernel (8 waves of 32 slots per lane).
constexpr int Q_MAX_WINDOW = 1024, Q_MAX_WAVE = 4096, Q_MAX_SPLIT = 16384;
// Whether a problem runs the q-split kernel: more than Q_MAX_WINDOW q-points, unless one wavefront per chain is asked for — by
// MCSAS_EXEC_WAVE, or by waves_per_chain = 1 where MCSAS_EXEC_AUTO leaves the choice.  (The pipeline has no kernel for such data, and
// none takes more than Q_MAX_SPLIT: plan creation refuses both.)
inline bool runs_q_split(int exec_mode, int waves_per_chain, int nq) {
    const bool wave_asked = exec_mode == MCSAS_EXEC_WAVE || (exec_mode == MCSAS_EXEC_AUTO && waves_per_chain == 1);
    return nq > Q_MAX_WINDOW && !wave_asked && exec_mode != MCSAS_EXEC_PIPELINE;
}
// A request that does not leave the mode to the plan — a start, a trace, a batch: MCSAS_EXEC_AUTO and MCSAS_EXEC_WAVE both mean one
// wavefront per chain, which takes up to Q_MAX_WAVE q-points.  Each caller refuses the other two answers in its own order and words.
enum WaveRequest { WAVE_RUNS, WAVE_NOT_ASKED, WAVE_TOO_MANY_Q };
inline WaveRequest wave_request(int exec_mode, int nq) {
    if (exec_mode != MCSAS_EXEC_AUTO && exec_mode != MCSAS_EXEC_WAVE) return WAVE_NOT_ASKED;
    return nq > Q_MAX_WAVE ? WAVE_TOO_MANY_Q : WAVE_RUNS;
}

#pragma GCC visibility pop

// ------------------------------------------------------------------------------ the data of a problem as the chains read them
// the weights and weighted data (weigh_points), padded with zeros, and their sums in the argument block.  Plan creation (mcsas_hip.hip)
// and the chains whose rows the caller evaluates (host_rows.hip) prepare them alike.  (Outside the hidden region above, and kept out of
// line: the library has always exported this constructor, and its list of symbols stays what it was.)
struct WeighedData {
    std::vector<double> w, wI, I;
    __attribute__((noinline)) WeighedData(const mcsas_problem *p, size_t qpad, mcsas::ChainArgs *a) : w(qpad, 0.), wI(qpad, 0.), I(qpad, 0.) {
        const WeighedSums s = weigh_points(p->intensity, p->sigma, p->nq, w.data(), wI.data(), I.data());
        a->nq = p->nq; a->qpad = (int)qpad; a->Sw = s.Sw; a->SI = s.SI; a->SII = s.SII; a->Ssig2 = s.Ssig2;
    }
};
