// mcsas_hip.hip — libmcsas_hip.so: C ABI (include/mcsas_hip.h) over the gfx950 chain kernels.  This unit holds the plans: their
// creation, start and trace, launches, fetches and batch launches, with the memory cache, the streams and the ABI queries.  What
// it decides without a device is host_decide.hip (the chain settings and the weights of every unit's chains among it), the one-shot
// analyses over plans are host_analyse.hip, the chains whose rows the caller evaluates host_rows.hip, several data sets fitted with one
// population host_sets.hip, the run-time compiler of model plug-ins host_plugin.hip, the small one-call entry points (model.calc, input
// preparation) host_calls.hip, McSAS.histogram() host_hist.hip; what they share is host_internal.h (the stop word and the wait that
// forwards McSAS.stop stand here, beside the cache the word comes from), and host_result.h writes every mcsas_result.
// Built only for MI355X (gfx950); there is no CPU path in here.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "host_decide.h" // host_internal.h, and of the kernel headers chain_wg.h and pipe_layout.h: geometry and argument blocks
#include "host_result.h"
#include "chain_wide.h" // WIDE_* constants only
#include "model_list.h" // MCSAS_FOR_MODELS: the built-in models

using namespace mcsas;

// ------------------------------------------------------------------------------ host helpers
int SmearDev::upload(const mcsas_problem *p, int stride, ModelArgs *m) {
    m->smear_nk = 0; m->smear_stride = 0; m->smear_locs_t = nullptr; m->smear_cw = nullptr;
    if (!active(p)) return MCSAS_OK;
    if (int rc = check(p)) return rc;
    const int K = p->smear_nk;
    std::vector<double> lt((size_t)K * stride), hcw(K);
    for (int k = 0; k < K; ++k)
        for (int i = 0; i < stride; ++i) lt[(size_t)k * stride + i] = p->smear_locs[(size_t)(i < p->nq ? i : 0) * K + k];
    for (int k = 0; k < K; ++k) {
        const double dl = k > 0 ? p->smear_q_offset[k] - p->smear_q_offset[k - 1] : 0.;
        const double dr = k + 1 < K ? p->smear_q_offset[k + 1] - p->smear_q_offset[k] : 0.;
        hcw[k] = 2. * (0.5 * (dl + dr)) * p->smear_weights[k];
    }
    HIPCHK(hipMalloc(&locs_t, sizeof(double) * lt.size()));
    HIPCHK(hipMalloc(&cw, sizeof(double) * K));
    HIPCHK(hipMemcpy(locs_t, lt.data(), sizeof(double) * lt.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(cw, hcw.data(), sizeof(double) * K, hipMemcpyHostToDevice));
    m->smear_nk = K; m->smear_stride = stride; m->smear_locs_t = locs_t; m->smear_cw = cw;
    for (size_t i = 0; i < lt.size(); ++i) m->qmax = std::max(m->qmax, std::fabs(lt[i]));
    return MCSAS_OK;
}

int select_device(int device) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(MCSAS_ENODEV, "no HIP device available");
    if (device >= n) return fail(MCSAS_ENODEV, "device %d requested, %d present", device, n);
    if (device >= 0) HIPCHK(hipSetDevice(device));
    return MCSAS_OK;
}

// ------------------------------------------------------------------------------ plan
// Device memory of a plan.  The big arrays (row cache, window buffers, replay streams: tens of MB) are allocations of their
// own; everything else — the data vectors, the chains' records and running sums, parameter sets, the windows' scalars and
// proposals, ~3 MB at config 2 — is carved out of 8 MB chunks, 256-byte aligned: a tick's blocks each touch a dozen of
// these small arrays before their first row, and packed into one 2 MB-aligned range they share a handful of page-table
// entries instead of one scattered 4 KB / 64 KB page per array (and a plan costs 6 hipMalloc calls instead of 25).
// Memory that plans give back is kept for the next plan (per device, exact size): a series of analyses — McSAS.calc() per data
// set, one plan each — otherwise pays ~3 ms of hipFree / hipHostFree per plan for 3.4 ms of kernels, plus as much for stream and
// pinned-memory creation.  Up to 4 GiB of device memory (MCSAS_HIP_CACHE_MB in the environment: another cap, 0 = none) stay parked;
// mcsas_hip_release_cached_memory() frees them.
struct MemCache {
    std::mutex mu;
    std::multimap<std::pair<int, size_t>, void *> dev;        // (device, bytes) -> free device blocks
    std::multimap<std::pair<unsigned, size_t>, void *> host;  // (flags, bytes) -> free pinned blocks
    std::map<int, hipStream_t> copy_stream;                   // per device: the non-blocking stream results come back on
    size_t dev_bytes = 0;
    // how much device memory may stay parked per process: 4 GiB, or MCSAS_HIP_CACHE_MB from the environment (0: nothing is kept —
    // for hosts whose own allocator (torch's, say) should see every byte this library is not using)
    size_t cap_bytes = (size_t)4 << 30;
    MemCache() {
        if (const char *e = getenv("MCSAS_HIP_CACHE_MB")) { char *end = nullptr; const long long mb = strtoll(e, &end, 10); if (end != e && mb >= 0) cap_bytes = (size_t)mb << 20; }
    }
};
static MemCache &mem_cache() { static MemCache c; return c; }
hipError_t cached_dev_malloc(void **p, size_t n) {
    int d = 0;
    hipError_t e = hipGetDevice(&d);
    if (e != hipSuccess) return e;
    {
        MemCache &c = mem_cache();
        std::lock_guard<std::mutex> lk(c.mu);
        auto it = c.dev.find({d, n});
        if (it != c.dev.end()) { *p = it->second; c.dev.erase(it); c.dev_bytes -= n; return hipSuccess; }
    }
    e = hipMalloc(p, n);
    if (e == hipErrorOutOfMemory) {                           // parked blocks of other sizes may be in the way
        { MemCache &c = mem_cache(); std::lock_guard<std::mutex> lk(c.mu); for (auto &kv : c.dev) hipFree(kv.second); c.dev.clear(); c.dev_bytes = 0; }
        (void)hipGetLastError();
        e = hipMalloc(p, n);
    }
    return e;
}
void cached_dev_free(void *p, size_t n, int d) {
    MemCache &c = mem_cache();
    std::lock_guard<std::mutex> lk(c.mu);
    if (c.dev_bytes + n <= c.cap_bytes) { c.dev.insert({{d, n}, p}); c.dev_bytes += n; }
    else hipFree(p);
}
hipError_t cached_host_malloc(void **p, size_t n, unsigned flags) {
    {
        MemCache &c = mem_cache();
        std::lock_guard<std::mutex> lk(c.mu);
        auto it = c.host.find({flags, n});
        if (it != c.host.end()) { *p = it->second; c.host.erase(it); return hipSuccess; }
    }
    return hipHostMalloc(p, n, flags);
}
void cached_host_free(void *p, size_t n, unsigned flags) {
    if (!p) return;
    MemCache &c = mem_cache();
    std::lock_guard<std::mutex> lk(c.mu);
    if (c.cap_bytes > 0 && c.host.size() < 64) c.host.insert({{flags, n}, p});
    else hipHostFree(p);
}
hipError_t cached_copy_stream(hipStream_t *st) {
    int d = 0;
    hipError_t e = hipGetDevice(&d);
    if (e != hipSuccess) return e;
    MemCache &c = mem_cache();
    std::lock_guard<std::mutex> lk(c.mu);
    auto it = c.copy_stream.find(d);
    if (it == c.copy_stream.end()) {
        hipStream_t s = nullptr;
        e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
        if (e != hipSuccess) return e;
        it = c.copy_stream.emplace(d, s).first;
    }
    *st = it->second;
    return hipSuccess;
}
hipError_t StopWord::make() {
    hipError_t e = cached_host_malloc((void **)&h, sizeof(int32_t), hipHostMallocMapped);
    if (e == hipSuccess) { *h = 0; e = hipHostGetDevicePointer((void **)&d, h, 0); }
    return e;
}
int wait_forwarding_stop(const char *who, hipEvent_t done, const volatile int32_t *caller_stop, int32_t *h_stop) {
    while (caller_stop) {                                // (no stop word: nothing to forward, plain wait below)
        hipError_t q = hipEventQuery(done);
        if (q == hipSuccess) break;
        if (q != hipErrorNotReady) return fail(MCSAS_EHIP, "%skernel failed: %s", who, hipGetErrorString(q));
        if (*caller_stop) *h_stop = 1;
        std::this_thread::sleep_for(std::chrono::microseconds(50));
    }
    HIPCHK(hipEventSynchronize(done));
    return MCSAS_OK;
}
extern "C" int mcsas_hip_release_cached_memory(void) {
    MemCache &c = mem_cache();
    std::lock_guard<std::mutex> lk(c.mu);
    for (auto &kv : c.dev) hipFree(kv.second);
    for (auto &kv : c.host) hipHostFree(kv.second);
    c.dev.clear(); c.host.clear(); c.dev_bytes = 0;
    return MCSAS_OK;
}

struct DevPool {
    static constexpr size_t CHUNK = (size_t)8 << 20, BIG = (size_t)2 << 20, ALIGN = 256;
    std::vector<std::pair<void *, size_t>> blocks;   // everything to give back
    int dev = 0;
    char *cur = nullptr;
    size_t left = 0;
    hipError_t get(void **out, size_t n) {
        *out = nullptr;
        n = (n ? n : 1);
        n = (n + ALIGN - 1) / ALIGN * ALIGN;
        void *p = nullptr;
        if (blocks.empty()) (void)hipGetDevice(&dev);
        if (n >= BIG) {
            hipError_t e = cached_dev_malloc(&p, n);
            if (e != hipSuccess) return e;
            blocks.push_back({p, n}); *out = p;
            return hipSuccess;
        }
        if (n > left) {                 // (the tail of the old chunk stays unused)
            hipError_t e = cached_dev_malloc(&p, CHUNK);
            if (e != hipSuccess) return e;
            blocks.push_back({p, (size_t)CHUNK}); cur = (char *)p; left = CHUNK;
        }
        *out = cur; cur += n; left -= n;
        return hipSuccess;
    }
    template <class T> hipError_t get(T **out, size_t n_bytes) { return get((void **)out, n_bytes); }
    void release() { for (auto &b : blocks) cached_dev_free(b.first, b.second, dev); blocks.clear(); cur = nullptr; left = 0; }
};

// What the analyses of one mcsas_hip_plan_launch_batch share, in one device block: the stop relay (one for the whole batch: a relay
// per analysis would multiply the chains' reads of host memory, chain_common.h: stop_requested), the argument blocks of the analyses
// and the chain table of the batch kernel, plus the pinned host word McSAS.stop is forwarded into and the staging copy of the block.
// Every plan of the batch holds a reference; a plan gives it up only once its own analysis is over (plan destroyed or launched
// again), so the last reference goes when every group of the batch has ended.
struct BatchShared {
    int dev = 0;
    size_t bytes = 0;
    char *d_block = nullptr;            // [0, 256): relay; then ChainArgs[n]; then ChainRef[chains]
    char *h_block = nullptr;            // pinned staging copy of d_block (the upload is asynchronous)
    StopWord stop;
    ~BatchShared() {
        if (d_block) cached_dev_free(d_block, bytes, dev);
        cached_host_free(h_block, bytes, hipHostMallocDefault);
    }
};

struct mcsas_plan {
    DevPool pool;
    mcsas_problem prob;
    ChainArgs args{};
    SmearDev smear;                     // device copy of the smearing tables (empty when off)
    int qpl = 0, waves = 1, use_cache = 1, dev = 0;
    bool wide = false;                  // more than 1024 q-points, one workgroup per chain with the q-points split over its waves (chain_wide.h)
    size_t lds_bytes = 0;
    double *d_q = nullptr, *d_w = nullptr, *d_wI = nullptr, *d_I = nullptr, *d_q3inv = nullptr;
    double *d_cache = nullptr, *d_replay = nullptr;
    double *d_start = nullptr;          // [n_reps][n_contrib][n_active], the layout of rset: the set every launch starts from (mcsas_hip_plan_set_start)
    bool has_start = false;             // ... while this holds; the buffer stays with the plan once made
    int32_t trace_capacity = 0;         // > 0: every launch runs the traced kernel and keeps this many moves per repetition (mcsas_hip_plan_set_trace)
    StopWord stop;                      // McSAS.stop as the kernels see it
    int32_t *d_stop_relay = nullptr;    // device memory, 16 bytes: the relayed stop word and the time stamp of the last look at h_stop (chain_common.h: stop_requested)
    hipStream_t stream = nullptr;
    bool enqueue_failed = false;        // a launch returned an error after it had put work on `stream`: nothing marks where that work ends
    WgGeom wg{};
    // whole-chip pipeline (exec_mode 3)
    int mode = MCSAS_EXEC_WAVE;
    PipeArgs pipe{};                    // (its pointers are the pipeline's workspace: make_pipeline_workspace)
    PipeArgs *d_pipeargs = nullptr;     // the argument block the tick kernels read (device copy)
    hipStream_t sCopy = nullptr;        // fetch(): results come back on a non-blocking stream of their own (a blocking copy would
                                        // wait for whatever else is queued on the null stream — another plan's launch)
    hipFunction_t plugin_fn = nullptr;  // the chain kernel of a run-time model plug-in for this plan's mode and q count (this device's module), else null
    static constexpr int RING = 64;
    hipEvent_t evS[RING] = {};
    // Result slots (mcsas_hip_plan_launch_slot / _fetch_slot): everything a finished analysis is read back from — parameter
    // sets, fits, per-chain outputs, the timing events, the host-visible "all chains done" word — exists MCSAS_PLAN_SLOTS times,
    // the workspaces (row cache, window buffers, chain records) once.  A slot is made on first use (make_slot); the kernels'
    // argument blocks point at the one that was last activated (plan_activate_slot).
    struct Slot {
        double *d_rset = nullptr, *d_fit = nullptr;
        ChainOut *d_out = nullptr;
        hipEvent_t ev0 = nullptr, ev1 = nullptr;
        int32_t *h_done = nullptr;      // pinned + mapped: the scan block of the last chain to finish writes the chain count into it
        int32_t *d_done_map = nullptr;  // ... and its device address
        PipeArgs *h_pipeargs = nullptr; // pinned staging copy of the tick kernels' argument block: the upload is a true asynchronous copy, so
                                        // launch() of one plan does not wait for another plan's work queued on the same stream
        bool launched = false, made = false;
        int ticks_launched = 0;
        double last_ms = 0.;
        int64_t last_steps = 0;
        // the batch (mcsas_hip_plan_launch_batch) whose launch wrote this slot, or null: its stop word is the one fetch() forwards to
        std::shared_ptr<BatchShared> batch_of;
        // the trace of the slot's last launch (mcsas_hip_plan_set_trace): one device block of its own, made by the first traced launch
        // of the slot, given back when the trace is cleared or resized and with the plan
        TraceArgs trace{};
        char *d_trace = nullptr;
        size_t trace_bytes = 0;
        bool traced = false;            // the launch that `launched` stands for ran the traced kernel
    };
    Slot slots[MCSAS_PLAN_SLOTS];
    int cur_slot = 0;
    Slot &cur() { return slots[cur_slot]; }
};

// the memory of result slot k (its three arrays come out of the plan's pool)
static int make_slot(mcsas_plan *pl, int k) {
    mcsas_plan::Slot &n = pl->slots[k];
    const size_t R = pl->prob.n_reps, N = pl->prob.n_contrib, P = pl->prob.n_active, qpad = pl->args.qpad;
    HIPCHK(pl->pool.get(&n.d_rset, sizeof(double) * R * N * P));
    HIPCHK(pl->pool.get(&n.d_fit, sizeof(double) * R * qpad));
    HIPCHK(pl->pool.get(&n.d_out, sizeof(ChainOut) * R));
    HIPCHK(hipMemset(n.d_out, 0, sizeof(ChainOut) * R));
    HIPCHK(hipEventCreate(&n.ev0)); HIPCHK(hipEventCreate(&n.ev1));
    if (pl->mode == MCSAS_EXEC_PIPELINE) {
        HIPCHK(cached_host_malloc((void **)&n.h_done, sizeof(int32_t), hipHostMallocMapped));
        *n.h_done = 0;
        HIPCHK(hipHostGetDevicePointer((void **)&n.d_done_map, n.h_done, 0));
    }
    n.made = true;
    return MCSAS_OK;
}

// make slot k (allocated on first use) the one the kernels write
static int plan_activate_slot(mcsas_plan *pl, int k) {
    if (k < 0 || k >= MCSAS_PLAN_SLOTS) return fail(MCSAS_EINVAL, "slot %d (0..%d)", k, MCSAS_PLAN_SLOTS - 1);
    mcsas_plan::Slot &n = pl->slots[k];
    if (!n.made) { int rc = make_slot(pl, k); if (rc) return rc; }
    pl->args.rset = n.d_rset; pl->args.fit = n.d_fit; pl->args.out = n.d_out;
    pl->pipe.n_done = n.d_done_map;
    pl->cur_slot = k;
    return MCSAS_OK;
}

// ------------------------------------------------------------------------------ the chain kernels
// A kernel is (family, given): given = the first attempt takes the plan's start (mcsas_hip_plan_set_start).  The lookups of the
// built-in models, one per model, family and given (kern_*.hip; all `void *(int qpl, bool flag)`, flag: with the row cache (wave
// families) / rows pulled from a queue (pipeline tick)); null where the family has no start form.
typedef void *KernelLookup(int qpl, bool flag);
#define DECL_K(m) KernelLookup mcsas_wave_kernel_m##m, mcsas_wave_kernel_given_m##m, mcsas_wave_batch_kernel_m##m, mcsas_wave_batch_kernel_given_m##m, \
                               mcsas_wg_kernel_m##m, mcsas_wide_kernel_m##m, mcsas_wide_kernel_given_m##m, mcsas_pipe_tick_kernel_m##m, \
                               mcsas_wave_trace_kernel_m##m, mcsas_wave_trace_kernel_given_m##m, mcsas_wide_trace_kernel_m##m, mcsas_wide_trace_kernel_given_m##m;
#define ROW_K(m) {{mcsas_wave_kernel_m##m, mcsas_wave_kernel_given_m##m}, {mcsas_wave_batch_kernel_m##m, mcsas_wave_batch_kernel_given_m##m}, \
                  {mcsas_wg_kernel_m##m, nullptr}, {mcsas_wide_kernel_m##m, mcsas_wide_kernel_given_m##m}, {mcsas_pipe_tick_kernel_m##m, nullptr}, \
                  {mcsas_wave_trace_kernel_m##m, mcsas_wave_trace_kernel_given_m##m}, {mcsas_wide_trace_kernel_m##m, mcsas_wide_trace_kernel_given_m##m}},
MCSAS_FOR_MODELS(DECL_K)
static constexpr KernelLookup *const BUILTIN[MCSAS_MODEL_COUNT][KF_COUNT][2] = {MCSAS_FOR_MODELS(ROW_K)};
#undef DECL_K
#undef ROW_K
static_assert(BUILTIN[MCSAS_MODEL_COUNT - 1][KF_COUNT - 1][0] != nullptr, "ROW_K: a pair of lookups per family of KernelFamily (too few leave the last one null)");
void *mcsas_pipe_reset_kernel();

// What a launch needs: the kernel (built-in models: the host handle of the __global__ function; plug-ins: the function of this
// device's module), the block size, and what the family takes after its argument block: its second argument, if any, and behind
// that, in the traced families, the slot's TraceArgs.
struct KernelRef {
    void *entry = nullptr;
    hipFunction_t plugin = nullptr;
    unsigned block = 0;
    FamilyInfo::Arg2 arg2 = FamilyInfo::ARG2_NONE;
    bool trace = false;
    const void *id() const { return plugin ? (const void *)plugin : entry; }
};
// Whether the plan's family has started and traced kernels: the wavefront-per-chain and the q-split family have, the workgroup-window
// kernel and the pipeline have none.  What mcsas_hip_plan_set_start and mcsas_hip_plan_set_trace refuse by, and a batch with `wide`.
static bool takes_start_and_trace(const mcsas_plan *pl) { return pl->mode == MCSAS_EXEC_WAVE || pl->wide; }
// the family of the plan's own launches; a batch (mcsas_hip_plan_launch_batch) runs the plan's chains in KF_WAVE_BATCH instead.  Either
// way a launch takes the started kernel of its family while the plan holds a start (mcsas_hip_plan_set_start gives one to plans of
// the wave and q-split families only), and a plan of either with a trace (mcsas_hip_plan_set_trace) the traced family.
static KernelFamily plan_family(const mcsas_plan *pl, bool traced) {
    if (!takes_start_and_trace(pl)) return pl->mode == MCSAS_EXEC_PIPELINE ? KF_PIPE_TICK : KF_WG;
    if (pl->wide) return traced ? KF_WIDE_TRACE : KF_WIDE;
    return traced ? KF_WAVE_TRACE : KF_WAVE;
}
static KernelFamily plan_family(const mcsas_plan *pl) { return plan_family(pl, pl->trace_capacity > 0); }
static int resolve_kernel(const mcsas_plan *pl, KernelFamily family, bool given, KernelRef *k) {
    const FamilyInfo &f = KERNEL_FAMILY[family];
    const int model = pl->prob.model_id;
    const bool flag = family == KF_PIPE_TICK ? pl->pipe.g.rowq != 0 : pl->use_cache != 0;
    *k = KernelRef{};
    k->block = family_block(family, pl->waves); k->arg2 = f.arg2; k->trace = f.trace;
    if (is_plugin_model(model)) {
        if (pl->plugin_fn && family == plan_family(pl) && !k->trace && !given) { k->plugin = pl->plugin_fn; return MCSAS_OK; }   // (looked up when the plan was made)
        return plugin_chain_function(model, family, pl->qpl, flag, given, &k->plugin);                           // (compiled on first use of this q count)
    }
    KernelLookup *const lookup = model >= 0 && model < MCSAS_MODEL_COUNT ? BUILTIN[model][family][given] : nullptr;
    k->entry = lookup ? lookup(pl->qpl, flag) : nullptr;
    if (!k->entry) return fail(MCSAS_EINVAL, "%sno %s%skernel for model %d qpl %d", family == KF_WAVE_BATCH ? "launch_batch: " : "", f.word, given ? "start " : "", model, pl->qpl);
    return MCSAS_OK;
}
// the kernel a launch of the plan takes now
static int launch_kernel_of(const mcsas_plan *pl, bool batch, KernelRef *k) {
    return resolve_kernel(pl, batch ? KF_WAVE_BATCH : plan_family(pl), pl->has_start, k);
}
// one launch of `grid` blocks; built-in kernels get their dynamic LDS limit raised when they need more than the default 64 KiB
static int launch_kernel(const KernelRef &k, unsigned grid, void **kargs, size_t lds, hipStream_t st) {
    if (k.plugin) HIPCHK(hipModuleLaunchKernel(k.plugin, grid, 1, 1, k.block, 1, 1, (unsigned)lds, st, kargs, nullptr));
    else HIPCHK(hipLaunchKernel(k.entry, dim3(grid), dim3(k.block), kargs, lds, st));
    return MCSAS_OK;
}
static int raise_lds_limit(const KernelRef &k, size_t lds) {
    if (k.entry && lds > 64 * 1024) HIPCHK(hipFuncSetAttribute(k.entry, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    return MCSAS_OK;
}

// waits for every launch of the plan still in flight, slot by slot; the first error, after every slot was waited for
static hipError_t wait_for_slots(mcsas_plan *pl) {
    hipError_t first = hipSuccess;
    for (mcsas_plan::Slot &sl : pl->slots)
        if (sl.launched && sl.ev1) { const hipError_t e = hipEventSynchronize(sl.ev1); if (first == hipSuccess) first = e; }
    return first;
}

extern "C" void mcsas_hip_plan_destroy(mcsas_plan *pl) {
    if (!pl) return;
    // (nothing of this plan may still be running when its memory goes back to the cache: hipFree used to wait, the cache does not)
    if (pl->enqueue_failed) {           // a launch that failed half-way left kernels behind no event of ours: wait for the stream (and the device)
        (void)hipSetDevice(pl->dev);
        (void)hipStreamSynchronize(pl->stream);
        (void)hipDeviceSynchronize();
        (void)hipGetLastError();
    }
    (void)wait_for_slots(pl);
    pl->pool.release();                 // every device array of the plan
    for (int i = 0; i < mcsas_plan::RING; ++i)
        if (pl->evS[i]) hipEventDestroy(pl->evS[i]);
    for (mcsas_plan::Slot &sl : pl->slots) {              // (a slot that was never made, or only half made, holds nulls)
        cached_host_free(sl.h_done, sizeof(int32_t), hipHostMallocMapped);
        cached_host_free(sl.h_pipeargs, sizeof(PipeArgs), hipHostMallocDefault);
        if (sl.d_trace) cached_dev_free(sl.d_trace, sl.trace_bytes, pl->dev);
        if (sl.ev0) hipEventDestroy(sl.ev0);
        if (sl.ev1) hipEventDestroy(sl.ev1);
    }
    delete pl;
}

// ------------------------------------------------------------------------------ plan creation
// the padded data vectors on the device
static int upload_data(mcsas_plan *pl, const mcsas_problem *p, int qpad) {
    ChainArgs &a = pl->args;
    const WeighedData h(p, qpad, &a);
    std::vector<double> hq(qpad);
    for (int i = 0; i < qpad; ++i) hq[i] = p->q[i < p->nq ? i : 0];
    const size_t vb = sizeof(double) * qpad;
    HIPCHK(pl->pool.get(&pl->d_q, vb)); HIPCHK(pl->pool.get(&pl->d_w, vb)); HIPCHK(pl->pool.get(&pl->d_wI, vb)); HIPCHK(pl->pool.get(&pl->d_I, vb));
    HIPCHK(hipMemcpy(pl->d_q, hq.data(), vb, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(pl->d_w, h.w.data(), vb, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(pl->d_wI, h.wI.data(), vb, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(pl->d_I, h.I.data(), vb, hipMemcpyHostToDevice));
    {   // 1 / q^3 (the branch-free sphere kernel's second reciprocal): the same two multiplications and the same correctly
        // rounded division the kernels used to make per block
        std::vector<double> hq3(qpad);
        for (int i = 0; i < qpad; ++i) hq3[i] = 1.0 / (hq[i] * hq[i] * hq[i]);
        HIPCHK(pl->pool.get(&pl->d_q3inv, vb));
        HIPCHK(hipMemcpy(pl->d_q3inv, hq3.data(), vb, hipMemcpyHostToDevice));
    }
    a.q = pl->d_q; a.w = pl->d_w; a.wI = pl->d_wI; a.I = pl->d_I;
    return MCSAS_OK;
}

// the intensity cache (`cache_rows` rows per chain, plus the spare one) and the replay streams
static int alloc_rows(mcsas_plan *pl, const mcsas_problem *p, int cache_rows) {
    const size_t R = p->n_reps;
    const bool wide_q = p->nq > Q_MAX_WINDOW;
    // The chains' row blocks must not all start at the same offset modulo the memory system's interleave: with N = 400 rows of
    // 4 KB a chain's block is 50 x 32 KB, every chain's row r sits at the same place in the channel pattern, and thousands of
    // chains walking their rows in step queue up on the same channels (measured: identical launches of 8192 chains at 3.7e8 or
    // 7.5e8 steps/s depending on whether the chains happened to run in step).  Spare rows make the block an odd number of rows.
    {
        int pad_rows = (cache_rows & 1) ? 0 : 1;
        if (const char *e = getenv("MCSAS_HIP_CACHE_PAD_ROWS")) pad_rows = atoi(e) < 0 ? 0 : atoi(e);     // (measurement knob)
        cache_rows += pad_rows;
    }
    size_t cache_bytes = sizeof(double) * R * (size_t)cache_rows * pl->args.qpad;
    int use_cache = p->cache_intensities;
    if (use_cache < 0 || pl->mode != MCSAS_EXEC_WAVE || wide_q) {
        size_t fr = 0, tot = 0;
        HIPCHK(hipMemGetInfo(&fr, &tot));
        use_cache = cache_bytes < fr / 2;
        if ((pl->mode != MCSAS_EXEC_WAVE || wide_q) && !use_cache) return fail(MCSAS_ENOMEM, "intensity cache (%zu MB) does not fit", cache_bytes >> 20);
    }
    pl->use_cache = use_cache;
    if (use_cache) HIPCHK(pl->pool.get(&pl->d_cache, cache_bytes));

    if (p->replay_stream) {
        HIPCHK(pl->pool.get(&pl->d_replay, sizeof(double) * R * (size_t)p->replay_len));
        HIPCHK(copy_replay(pl->d_replay, p, R));
    }
    ChainArgs &a = pl->args;
    a.cache = pl->d_cache; a.cache_rows = cache_rows;
    a.replay = pl->d_replay; a.replay_len = p->replay_len;
    return MCSAS_OK;
}

// the rest of the kernels' argument block: the model, the problem's settings and the stop word with its relay
static int fill_chain_args(mcsas_plan *pl, const mcsas_problem *p, const ModelArgs &margs) {
    HIPCHK(pl->stop.make());
    ChainArgs &a = pl->args;
    a.model = margs;
    fill_chain_settings(p, &a);
    a.pad0 = p->reserved0;                               // (0 in the release library: validate_problem)
    a.stop_flag = pl->stop.d;
    HIPCHK(pl->pool.get(&pl->d_stop_relay, 16));
    a.stop_relay = pl->d_stop_relay;
    return MCSAS_OK;
}

// the plan's kernel and its dynamic LDS.  The wavefront and q-split kernels of a built-in model are looked up here, so that a shape
// without one is refused with the plan; a plug-in's kernel is compiled and kept (plugin_fn); the workgroup and pipeline kernels of
// the built-in models are looked up by the launch.
static int choose_kernel(mcsas_plan *pl) {
    const int model = pl->prob.model_id, int_div = pl->args.model.int_div;
    const KernelFamily family = plan_family(pl);
    if (is_plugin_model(model) || family == KF_WAVE || family == KF_WIDE) {
        KernelRef k;
        if (int rc = resolve_kernel(pl, family, false, &k)) return rc;
        pl->plugin_fn = k.plugin;
    }
    if (family == KF_WAVE) {
        pl->lds_bytes = sizeof(double) * (4 * (size_t)pl->args.qpad + table_doubles_block(model, int_div, 1));
    } else if (family == KF_WIDE) {
        // partial sums, the model's tables and one row scratch per wave; q and 1/q^3 as well when they fit (ChainArgs::pad1)
        const size_t base = sizeof(double) * ((size_t)WIDE_PART_DOUBLES + table_doubles_block(model, int_div, pl->waves));
        const size_t with_q = base + sizeof(double) * 2 * (size_t)pl->args.qpad;
        pl->args.pad1 = with_q <= 150 * 1024 ? 1 : 0;
        pl->lds_bytes = pl->args.pad1 ? with_q : base;
    } else if (family == KF_WG) {
        pl->lds_bytes = pl->wg.lds_bytes;
    } else {
        pl->lds_bytes = std::max(pl->pipe.g.prod_lds, pl->pipe.g.scan_lds);
    }
    return MCSAS_OK;
}

// the pipeline's workspace: chain records, window buffers, proposals, the tick kernels' argument block
static int make_pipeline_workspace(mcsas_plan *pl) {
    const size_t R = pl->prob.n_reps, N = pl->prob.n_contrib, qpad = pl->args.qpad;
    PipeArgs &pa = pl->pipe;
    const size_t Kb = pa.g.kb;
    pa.c = pl->args;
    HIPCHK(pl->pool.get(&pa.chains, sizeof(PipeChain) * R));
    HIPCHK(pl->pool.get(&pl->d_pipeargs, sizeof(PipeArgs)));
    HIPCHK(pl->pool.get(&pa.ft, sizeof(double) * R * qpad)); HIPCHK(pl->pool.get(&pa.wft, sizeof(double) * R * qpad));
    HIPCHK(pl->pool.get(&pa.slot_of, sizeof(int32_t) * R * N)); HIPCHK(pl->pool.get(&pa.stage_slot, sizeof(int32_t) * R * 2 * Kb));
    HIPCHK(pl->pool.get(&pa.dwin, sizeof(double) * R * 2 * Kb * qpad));
    HIPCHK(pl->pool.get(&pa.gwin, sizeof(double) * R * 2 * Kb * pa.g.w));
    HIPCHK(pl->pool.get(&pa.scal, sizeof(double) * R * 2 * Kb * 4));
    HIPCHK(pl->pool.get(&pa.row_valid, sizeof(int32_t) * R * N));
    HIPCHK(hipMemset(pa.row_valid, 0, sizeof(int32_t) * R * N));
    HIPCHK(pl->pool.get(&pa.rowq, sizeof(int32_t) * R * 2));
    HIPCHK(hipMemset(pa.rowq, 0, sizeof(int32_t) * R * 2));
    HIPCHK(pl->pool.get(&pa.pval, sizeof(double) * R * 2 * Kb * MCSAS_MAX_ACTIVE));
    HIPCHK(pl->pool.get(&pa.povf, sizeof(int32_t) * R * 2 * Kb));
    HIPCHK(hipMemset(pa.povf, 0, sizeof(int32_t) * R * 2 * Kb));
    for (int i = 0; i < mcsas_plan::RING; ++i)
        HIPCHK(hipEventCreateWithFlags(&pl->evS[i], hipEventDisableTiming));
    HIPCHK(pl->pool.get(&pa.n_done_dev, sizeof(int32_t)));                  // (n_done: the active slot's, plan_activate_slot)
    pa.tick = 0; pa.timeline = nullptr; pa.timeline_tick = -100;
#ifdef MCSAS_STAMPS
    if (const char *e = getenv("MCSAS_TIMELINE_TICK")) {
        pa.timeline_tick = atoi(e);
        HIPCHK(pl->pool.get(&pa.timeline, sizeof(uint64_t) * 8 * PIPE_TL_WORDS * (R + R * pa.g.prod_blocks_y)));
        HIPCHK(hipMemset(pa.timeline, 0, sizeof(uint64_t) * 8 * PIPE_TL_WORDS * (R + R * pa.g.prod_blocks_y)));
    }
#endif
    return MCSAS_OK;
}

extern "C" int mcsas_hip_plan_create(const mcsas_problem *p, mcsas_plan **out) {
    if (!p || !out) return fail(MCSAS_EINVAL, "null argument");
    *out = nullptr;
    int rc = validate_problem(p);
    if (rc) return rc;
    ModelArgs margs;
    rc = fill_model_args(p, &margs);
    if (rc) return rc;
    for (int c = 0; c < p->n_active; ++c)
        if (p->gen_kind[c] < 0 || p->gen_kind[c] > 3) return fail(MCSAS_EINVAL, "gen_kind[%d]=%d", c, p->gen_kind[c]);
    DeviceGuard dev_guard;
    rc = select_device(p->device);
    if (rc) return rc;

    std::unique_ptr<mcsas_plan, decltype(&mcsas_hip_plan_destroy)> pl(new mcsas_plan(), mcsas_hip_plan_destroy);     // (every error return below gives back what the plan holds by then)
    pl->prob = *p;
    pl->prob.q = pl->prob.intensity = pl->prob.sigma = nullptr;     // host arrays are not retained
    pl->prob.replay_stream = nullptr;
    pl->prob.smear_locs = pl->prob.smear_q_offset = pl->prob.smear_weights = nullptr;
    hipGetDevice(&pl->dev);

    int n_cus = 256;
    { int v = 0; if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, pl->dev) == hipSuccess && v > 0) n_cus = v; }
    size_t free_bytes = SIZE_MAX;
    if (p->exec_mode == MCSAS_EXEC_AUTO && p->waves_per_chain < 1) { size_t fr = 0, tot = 0; if (hipMemGetInfo(&fr, &tot) == hipSuccess) free_bytes = fr; }
    PlanShape sh;
    rc = decide_shape(p, margs, n_cus, free_bytes, tune_word(p), &sh);
    if (rc) return rc;
    pl->qpl = sh.qpl; pl->wide = sh.wide; pl->waves = sh.waves; pl->mode = sh.mode; pl->wg = sh.wg; pl->pipe.g = sh.pipe;

    // (the order of the pool's allocations below is the packing the comment above MemCache describes)
    rc = pl->smear.upload(p, sh.qpad, &margs);
    if (!rc) rc = upload_data(pl.get(), p, sh.qpad);
    if (!rc) rc = plan_activate_slot(pl.get(), 0);
    if (!rc) rc = alloc_rows(pl.get(), p, sh.cache_rows);
    if (!rc) rc = fill_chain_args(pl.get(), p, margs);
    if (!rc) rc = choose_kernel(pl.get());
    if (!rc && pl->mode == MCSAS_EXEC_PIPELINE) rc = make_pipeline_workspace(pl.get());
    if (rc) return rc;
    if (pl->lds_bytes > 160 * 1024) return fail(MCSAS_EINVAL, "LDS need %zu B > 160 KiB", pl->lds_bytes);
    *out = pl.release();
    return MCSAS_OK;
}

extern "C" int mcsas_hip_plan_reseed(mcsas_plan *pl, uint64_t seed, int32_t rep_offset) {
    if (!pl) return fail(MCSAS_EINVAL, "null plan");
    pl->args.seed = seed; pl->args.rep_offset = rep_offset;
    return MCSAS_OK;
}

// The set every later launch of the plan starts its repetitions from (include/mcsas_hip.h), kept on the device in the layout of rset;
// a launch copies it into its slot's rset on the launch stream and runs the started form of the plan's kernel, whose first attempt reads
// it where the cold one generates a set (chain_body.inc: GIVEN).  The wavefront-per-chain and the q-split kernels have such a form; the
// workgroup-window kernel (up to 1024 q-points) and the pipeline have none, and their plans refuse.
extern "C" int mcsas_hip_plan_set_start(mcsas_plan *pl, const double *start, int32_t rep_stride, int32_t rep_first) {
    if (!pl) return fail(MCSAS_EINVAL, "set_start: null plan");
    if (!start) { pl->has_start = false; return MCSAS_OK; }
    if (!takes_start_and_trace(pl))
        return fail(MCSAS_EINVAL, "set_start: the plan runs in exec_mode %d (%s) with %d q-points; a start needs exec_mode = MCSAS_EXEC_WAVE (%d), or MCSAS_EXEC_WORKGROUP (%d) with more than %d q-points",
                    pl->mode, exec_mode_name(pl->mode), pl->prob.nq, MCSAS_EXEC_WAVE, MCSAS_EXEC_WORKGROUP, Q_MAX_WINDOW);
    const size_t R = pl->prob.n_reps, N = pl->prob.n_contrib, P = pl->prob.n_active;
    if (rep_first < 0 || (int64_t)rep_first + (int64_t)R > (int64_t)rep_stride)
        return fail(MCSAS_EINVAL, "set_start: repetitions %d..%lld of a start with %d columns", rep_first, (long long)rep_first + (long long)R - 1, rep_stride);
    if (int rc = check_start_finite("set_start", start, N, P, (size_t)rep_stride, (size_t)rep_first, R)) return rc;
    std::vector<double> hr(R * N * P);
    for (size_t r = 0; r < R; ++r)
        for (size_t i = 0; i < N * P; ++i) hr[r * N * P + i] = start[i * (size_t)rep_stride + (size_t)rep_first + r];
    DeviceGuard dev_guard;
    HIPCHK(hipSetDevice(pl->dev));
    HIPCHK(wait_for_slots(pl));                           // (a launch still in flight may not have made its copy of the previous start yet)
    if (!pl->d_start) HIPCHK(pl->pool.get(&pl->d_start, sizeof(double) * hr.size()));
    HIPCHK(hipMemcpy(pl->d_start, hr.data(), sizeof(double) * hr.size(), hipMemcpyHostToDevice));
    pl->has_start = true;
    return MCSAS_OK;
}
// the slot's rset takes the start ahead of the kernel, on the launch stream
static int enqueue_start(mcsas_plan *pl, hipStream_t st) {
    const size_t bytes = sizeof(double) * (size_t)pl->prob.n_reps * pl->prob.n_contrib * pl->prob.n_active;
    HIPCHK(hipMemcpyAsync(pl->cur().d_rset, pl->d_start, bytes, hipMemcpyDeviceToDevice, st));
    return MCSAS_OK;
}

// ------------------------------------------------------------------------------ the trace of a wave or q-split plan (include/mcsas_hip.h)
static void drop_slot_trace(mcsas_plan *pl, mcsas_plan::Slot &sl) {
    if (sl.d_trace) cached_dev_free(sl.d_trace, sl.trace_bytes, pl->dev);
    sl.d_trace = nullptr; sl.trace_bytes = 0; sl.trace = TraceArgs{}; sl.traced = false;
}
// the slot's trace block for the plan's capacity: [step | chisq | values | chisq0], made on the slot's first traced launch
static int make_slot_trace(mcsas_plan *pl, mcsas_plan::Slot &sl) {
    if (sl.d_trace && sl.trace.capacity == pl->trace_capacity) return MCSAS_OK;
    drop_slot_trace(pl, sl);
    const TraceLayout at(pl->prob.n_reps, (size_t)pl->trace_capacity, pl->prob.n_active);
    HIPCHK(cached_dev_malloc((void **)&sl.d_trace, at.dev_bytes));
    sl.trace_bytes = at.dev_bytes;
    sl.trace.step = (int64_t *)(sl.d_trace + at.step);
    sl.trace.chisq = (double *)(sl.d_trace + at.chisq);
    sl.trace.values = (double *)(sl.d_trace + at.values);
    sl.trace.chisq0 = (double *)(sl.d_trace + at.chisq0);
    sl.trace.capacity = pl->trace_capacity; sl.trace.pad = 0;
    return MCSAS_OK;
}

extern "C" int mcsas_hip_plan_set_trace(mcsas_plan *pl, int32_t capacity) {
    if (!pl) return fail(MCSAS_EINVAL, "set_trace: null plan");
    if (capacity < 0) return fail(MCSAS_EINVAL, "set_trace: capacity %d (>= 1, or 0 to clear the trace)", (int)capacity);
    if (capacity > 0) {
        if (!takes_start_and_trace(pl))
            return fail(MCSAS_EINVAL, "set_trace: the plan runs in exec_mode %d (%s); a trace needs exec_mode = MCSAS_EXEC_WAVE (%d)", pl->mode, exec_mode_name(pl->mode), MCSAS_EXEC_WAVE);
        const size_t R = pl->prob.n_reps, P = pl->prob.n_active;
        if (TraceLayout::too_large(R, (size_t)capacity, P))
            return fail(MCSAS_EINVAL, "set_trace: %d repetitions x capacity %d x %zu bytes per move exceed 2 GiB", pl->prob.n_reps, (int)capacity, TraceLayout(R, 0, P).move_bytes);
    }
    DeviceGuard dev_guard;
    HIPCHK(hipSetDevice(pl->dev));
    if (capacity != pl->trace_capacity) {
        HIPCHK(wait_for_slots(pl));                       // (a launch still in flight writes the blocks that go back to the cache here)
        for (mcsas_plan::Slot &sl : pl->slots) drop_slot_trace(pl, sl);
    }
    if (capacity > 0 && !is_plugin_model(pl->prob.model_id)) {   // a shape without a traced kernel is refused here, as the plan's own is at its creation
        KernelRef k;
        if (int rc = resolve_kernel(pl, plan_family(pl, true), pl->has_start, &k)) return rc;
    }
    pl->trace_capacity = capacity;
    return MCSAS_OK;
}

extern "C" int mcsas_hip_plan_fetch_trace(mcsas_plan *pl, int32_t slot, mcsas_trace *tr) {
    if (!pl) return fail(MCSAS_EINVAL, "fetch_trace: null plan");
    if (pl->trace_capacity < 1) return fail(MCSAS_EINVAL, "fetch_trace: the plan has no trace (mcsas_hip_plan_set_trace)");
    if (int rc = check_trace_arrays("fetch_trace", tr)) return rc;
    if (tr->capacity != pl->trace_capacity) return fail(MCSAS_EINVAL, "fetch_trace: trace capacity %d, the plan's is %d", (int)tr->capacity, (int)pl->trace_capacity);
    if (slot < 0 || slot >= MCSAS_PLAN_SLOTS) return fail(MCSAS_EINVAL, "fetch_trace: slot %d (0..%d)", (int)slot, MCSAS_PLAN_SLOTS - 1);
    mcsas_plan::Slot &s = pl->slots[slot];
    if (!s.launched || !s.traced || !s.d_trace) return fail(MCSAS_EINVAL, "fetch_trace: slot %d holds no traced launch", (int)slot);
    DeviceGuard dev_guard;
    HIPCHK(hipSetDevice(pl->dev));
    HIPCHK(hipEventSynchronize(s.ev1));
    const size_t R = pl->prob.n_reps, K = (size_t)pl->trace_capacity, P = pl->prob.n_active;
    std::vector<ChainOut> ho(R);
    HIPCHK(hipMemcpy(ho.data(), s.d_out, sizeof(ChainOut) * R, hipMemcpyDeviceToHost));
    std::vector<char> h(TraceLayout(R, K, P).host_bytes);
    HIPCHK(hipMemcpy(h.data(), s.d_trace, h.size(), hipMemcpyDeviceToHost));
    trace_transpose(h.data(), R, K, P, ho.data(), tr);
    return MCSAS_OK;
}

// marks the plans of a launch that returns early: work of theirs is on the stream that no end event covers (mcsas_hip_plan_destroy)
struct FailGuard {
    mcsas_plan *const *plans; int n; bool ok = false;
    ~FailGuard() { if (!ok) for (int i = 0; i < n; ++i) plans[i]->enqueue_failed = true; }
};

static int pipeline_launch(mcsas_plan *pl, const KernelRef &tick, hipStream_t st) {
    mcsas_plan::Slot &s = pl->cur();
    PipeArgs &pa = pl->pipe;
    pa.c = pl->args;                                     // picks up reseed()
    pa.c.cache_rows = pl->args.cache_rows;
    const int R = pl->prob.n_reps, Kb = pa.g.kb;
    void *reset = mcsas_pipe_reset_kernel();
    const size_t lds = std::max(pa.g.prod_lds, pa.g.scan_lds);
    if (int rc = raise_lds_limit(tick, lds)) return rc;
    *s.h_done = 0;
    HIPCHK(hipMemsetAsync(pa.n_done_dev, 0, sizeof(int32_t), st));
    pa.tick = 0;
    if (!s.h_pipeargs) HIPCHK(cached_host_malloc((void **)&s.h_pipeargs, sizeof(PipeArgs), hipHostMallocDefault));
    *s.h_pipeargs = pa;                                  // (the previous launch's upload has completed: fetch() or the caller waited for it)
    HIPCHK(hipMemcpyAsync(pl->d_pipeargs, s.h_pipeargs, sizeof(PipeArgs), hipMemcpyHostToDevice, st));
    HIPCHK(hipEventRecord(s.ev0, st));
    {
        void *ka[] = {(void *)&pl->d_pipeargs};
        HIPCHK(hipLaunchKernel(reset, dim3((R + 63) / 64), dim3(64), ka, 0, st));
    }
    const long long max_ticks = pipeline_tick_budget(pl->prob.max_iter, pl->prob.max_retries, Kb);     // worst case: every attempt runs to max_iter
    // scan blocks + producer blocks (chain-major; 8 XCD classes of ceil(R/8) chains each with diagnostic bit 128)
    const dim3 grid((MCSAS_TUNE_BITS(pl->args) & 128) ? R + 8 * ((R + 7) / 8) * pa.g.prod_blocks_y : R + R * pa.g.prod_blocks_y);
    PipeHot hot{};
    hot.q = pa.c.q; hot.w = pa.c.w; hot.wI = pa.c.wI; hot.chains = pa.chains;
    hot.n_reps = pa.c.n_reps; hot.n_contrib = pa.c.n_contrib; hot.n_active = pa.c.model.n_active; hot.qpad = pa.c.qpad;
    hot.kb = pa.g.kb; hot.prod_blocks_y = pa.g.prod_blocks_y; hot.w_sub = pa.g.w; hot.max_iter = pa.c.max_iter;
    hot.q3inv = pl->d_q3inv;
    long long t = -1;                                    // launch t = {SCAN(t), PROD(t+1)}
    for (; t < max_ticks; ++t) {
        if (t >= mcsas_plan::RING && (t % 16) == 0) {
            // throttle: stay at most ~RING ticks ahead of the GPU, forward the stop word, leave when all chains are done
            HIPCHK(hipEventSynchronize(pl->evS[((t - mcsas_plan::RING) / 16) % mcsas_plan::RING]));
            if (pl->prob.stop && *pl->prob.stop) *pl->stop.h = 1;
            if (*(volatile int32_t *)s.h_done >= R) break;
        }
        int32_t tk = (int32_t)t, stop_now = (pl->prob.stop && *(volatile int32_t *)pl->prob.stop) ? 1 : 0;
        void *ka[] = {(void *)&pl->d_pipeargs, (void *)&tk, (void *)&stop_now, (void *)&hot};
        if (int rc = launch_kernel(tick, grid.x, ka, lds, st)) return rc;
        if (t >= 0 && (t % 16) == 0) HIPCHK(hipEventRecord(pl->evS[(t / 16) % mcsas_plan::RING], st));
    }
    s.ticks_launched = (int)t;
    HIPCHK(hipEventRecord(s.ev1, st));
    return MCSAS_OK;
}

extern "C" int mcsas_hip_plan_launch_slot(mcsas_plan *pl, void *hip_stream, int32_t slot) {
    if (!pl) return fail(MCSAS_EINVAL, "null plan");
    DeviceGuard dev_guard;
    HIPCHK(hipSetDevice(pl->dev));
    if (int rc = plan_activate_slot(pl, slot)) return rc;
    mcsas_plan::Slot &s = pl->cur();
    hipStream_t st = (hipStream_t)hip_stream;
    // The slots of a plan share its workspaces (row cache, chain records, window buffers, argument block): an analysis must not start
    // before the other slots' analyses have ended.  On one stream that is the stream's order; launched on ANOTHER stream this one waits
    // for their end events (a no-op when they are complete).  This slot's own previous analysis must be over before its pinned
    // argument block is rewritten.
    for (int k = 0; k < MCSAS_PLAN_SLOTS; ++k)
        if (k != pl->cur_slot && pl->slots[k].launched && pl->slots[k].ev1) HIPCHK(hipStreamWaitEvent(st, pl->slots[k].ev1, 0));
    if (s.launched && s.ev1) HIPCHK(hipEventSynchronize(s.ev1));
    s.batch_of.reset();
    *pl->stop.h = (pl->prob.stop && *pl->prob.stop) ? 1 : 0;
    pl->stream = st;
    if (pl->mode != MCSAS_EXEC_PIPELINE) HIPCHK(hipMemsetAsync(pl->d_stop_relay, 0, 16, st));   // (the pipeline's ticks get McSAS.stop as a kernel argument)
    FailGuard guard{&pl, 1};                              // (any error return below leaves work on `st` that no end event covers)
    KernelRef k;
    if (int rc = launch_kernel_of(pl, false, &k)) return rc;
    if (pl->mode == MCSAS_EXEC_PIPELINE) {
        if (int rc = pipeline_launch(pl, k, st)) return rc;
    } else {
        // the argument block by value, then what the family takes besides (a plug-in: the same arguments, through its code-object module)
        if (k.trace) { if (int rc = make_slot_trace(pl, s)) return rc; }
        void *kargs[3] = {(void *)&pl->args, nullptr, nullptr};
        int nk = 1;
        if (k.arg2 == FamilyInfo::ARG2_WG) kargs[nk++] = (void *)&pl->wg;
        else if (k.arg2 == FamilyInfo::ARG2_Q3INV) kargs[nk++] = (void *)&pl->d_q3inv;
        if (k.trace) kargs[nk++] = (void *)&s.trace;
        if (int rc = raise_lds_limit(k, pl->lds_bytes)) return rc;
        HIPCHK(hipEventRecord(s.ev0, st));
        if (pl->has_start) { if (int rc = enqueue_start(pl, st)) return rc; }
        if (int rc = launch_kernel(k, (unsigned)pl->prob.n_reps, kargs, pl->lds_bytes, st)) return rc;
        HIPCHK(hipEventRecord(s.ev1, st));
        s.traced = k.trace;
    }
    s.launched = true; guard.ok = true;
    return MCSAS_OK;
}

extern "C" int mcsas_hip_plan_launch(mcsas_plan *pl, void *hip_stream) { return mcsas_hip_plan_launch_slot(pl, hip_stream, 0); }

extern "C" int mcsas_hip_plan_fetch_slot(mcsas_plan *pl, int32_t slot, mcsas_result *res) {
    if (!pl) return fail(MCSAS_EINVAL, "null plan");
    DeviceGuard dev_guard;
    HIPCHK(hipSetDevice(pl->dev));
    if (int rc = plan_activate_slot(pl, slot)) return rc;
    mcsas_plan::Slot &s = pl->cur();
    if (!s.launched) return fail(MCSAS_EINVAL, "plan was not launched");
    if (res && res->struct_size != sizeof(mcsas_result))
        return fail(MCSAS_EINVAL, "mcsas_result size %u, library expects %zu", res->struct_size, sizeof(mcsas_result));
    // wait, forwarding the caller's stop word to the device-visible one (McSAS.stop, mcsas.py:357)
    if (int rc = wait_forwarding_stop("", s.ev1, pl->prob.stop, s.batch_of ? s.batch_of->stop.h : pl->stop.h)) return rc;
    if (!pl->sCopy) HIPCHK(cached_copy_stream(&pl->sCopy));      // (one per device, shared by every plan)
    // device -> host on the copy stream (the data is complete: ev1 has passed)
    auto d2h = [&](void *dst, const void *src, size_t n) -> hipError_t {
        hipError_t e = hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToHost, pl->sCopy);
        return e != hipSuccess ? e : hipStreamSynchronize(pl->sCopy);
    };
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, s.ev0, s.ev1));
    s.last_ms = ms;
    const size_t R = pl->prob.n_reps, N = pl->prob.n_contrib, P = pl->prob.n_active, Q = pl->prob.nq, qpad = pl->args.qpad;
    if (pl->mode == MCSAS_EXEC_PIPELINE && *(volatile int32_t *)s.h_done < (int32_t)R)
        return fail(MCSAS_EHIP, "pipeline: %d of %zu chains finished within the %d ticks that were launched",
                    (int)*(volatile int32_t *)s.h_done, R, s.ticks_launched + 1);
    std::vector<ChainOut> ho(R);
    HIPCHK(d2h(ho.data(), s.d_out, sizeof(ChainOut) * R));
    int64_t steps = 0; int ovf = 0;
    for (size_t r = 0; r < R; ++r) { steps += ho[r].total_steps; ovf |= ho[r].stream_overflow; }
    s.last_steps = steps;
#ifdef MCSAS_STAMPS
    {
        static const char *names[20] = {"rows+dot+reduce", "B1 wait", "decide", "B2 wait", "apply", "sub-windows", "accepted", "-",
                                        "prod rows", "prod barrier", "prod gram", "prod blocks",
                                        "prologue", "epilogue", "window ticks", "block total", "gap between blocks (10ns)", "gaps", "in block (10ns)", "-"};
        for (size_t r = 0; r < R && r < 2; ++r) {
            fprintf(stderr, "[mcsas stamps] rep %zu (wave 0 cycles):", r);
            for (int i = 0; i < 20; ++i) fprintf(stderr, " %s=%lld", names[i], (long long)ho[r].dbg[i]);
            fprintf(stderr, "\n");
        }
        if (pl->pipe.timeline) {
            const size_t nb = R + R * pl->pipe.g.prod_blocks_y;
            std::vector<uint64_t> tl(nb * 8 * PIPE_TL_WORDS);
            HIPCHK(d2h(tl.data(), pl->pipe.timeline, tl.size() * 8));
            uint64_t t0 = ~0ull;
            const size_t TW = PIPE_TL_WORDS;
            for (size_t i = 0; i < nb * 8; ++i) if (tl[i * TW] && tl[i * TW] < t0) t0 = tl[i * TW];
            fprintf(stderr, "[mcsas timeline] tick %d: block wave start_us end_us hw_id xcc\n", pl->pipe.timeline_tick);
            for (size_t i = 0; i < nb * 8; ++i)
                if (tl[i * TW]) {
                    fprintf(stderr, "[mcsas timeline] %zu %zu %.2f %.2f %llx %llu", i / 8, i % 8, (tl[i * TW] - t0) * 0.01, (tl[i * TW + 1] - t0) * 0.01,
                            (unsigned long long)tl[i * TW + 2], (unsigned long long)tl[i * TW + 3]);
                    for (size_t m = 4; m < TW; ++m) fprintf(stderr, " %.2f", tl[i * TW + m] ? (tl[i * TW + m] - t0) * 0.01 : 0.0);
                    fprintf(stderr, "\n");
                }
        }
        fprintf(stderr, "[mcsas stamps] per rep: in-block us / gap us:");
        for (size_t r = 0; r < R; ++r) fprintf(stderr, " %.0f/%.0f", ho[r].dbg[18] * 0.01, ho[r].dbg[16] * 0.01);
        fprintf(stderr, "\n");
    }
#endif
    if (res) {
        if (res->contribs) {
            std::vector<double> hr(R * N * P);
            HIPCHK(d2h(hr.data(), s.d_rset, sizeof(double) * hr.size()));
            result_put_sets(res, hr.data(), N, P, R, 0, R);
        }
        if (res->fit) {
            std::vector<double> hf(R * qpad);
            HIPCHK(d2h(hf.data(), s.d_fit, sizeof(double) * hf.size()));
            result_put_fit(res, hf.data(), qpad, Q, R, 0, R);
        }
        for (size_t r = 0; r < R; ++r) result_put_row(res, r, ho[r]);
    }
    if (ovf) return fail(MCSAS_ESTREAM, "replay stream exhausted (replay_len=%lld)", (long long)pl->prob.replay_len);
    return MCSAS_OK;
}

extern "C" int mcsas_hip_plan_fetch(mcsas_plan *pl, mcsas_result *res) { return mcsas_hip_plan_fetch_slot(pl, 0, res); }

extern "C" int mcsas_hip_plan_info(mcsas_plan *pl, int32_t info[8]) {
    if (!pl || !info) return fail(MCSAS_EINVAL, "null argument");
    memset(info, 0, sizeof(int32_t) * 8);
    info[0] = pl->mode; info[1] = pl->waves; info[2] = pl->qpl;
    info[3] = pl->mode == MCSAS_EXEC_PIPELINE ? pl->pipe.g.kb : (pl->mode == MCSAS_EXEC_WORKGROUP && !pl->wide ? pl->wg.window : 1);
    info[4] = pl->mode == MCSAS_EXEC_PIPELINE ? pl->cur().ticks_launched + 2 : 1;
    info[5] = pl->use_cache;
    return MCSAS_OK;
}

extern "C" int mcsas_hip_plan_last_ms(mcsas_plan *pl, double *ms) {
    if (!pl || !ms) return fail(MCSAS_EINVAL, "null argument");
    *ms = pl->cur().last_ms;
    return MCSAS_OK;
}
extern "C" int mcsas_hip_plan_total_steps(mcsas_plan *pl, int64_t *steps) {
    if (!pl || !steps) return fail(MCSAS_EINVAL, "null argument");
    *steps = pl->cur().last_steps;
    return MCSAS_OK;
}

// ------------------------------------------------------------------------------ several analyses in one launch
// One chain_wave_batch_kernel launch per group of plans that run the same kernel (model, q slots per lane, row cache, start or not): block b runs
// chain table entry b, i.e. one repetition of one plan, with that plan's own argument block.  A chain computes exactly what it
// computes in the plan's own launch; the plans only share the launch and the stop relay.
extern "C" int mcsas_hip_plan_launch_batch(mcsas_plan *const *plans, int32_t n, void *hip_stream) {
    if (!plans || n < 1) return fail(MCSAS_EINVAL, "launch_batch: needs n >= 1 plans (n = %d)", (int)n);
    for (int i = 0; i < n; ++i) {
        const mcsas_plan *pl = plans[i];
        if (!pl) return fail(MCSAS_EINVAL, "launch_batch: plan %d is null", i);
        if (!takes_start_and_trace(pl) || pl->wide)                          // (of the two such families, the wavefront-per-chain one)
            return fail(MCSAS_EINVAL, "launch_batch: plan %d runs in exec_mode %d; a batch takes wavefront-per-chain plans only (exec_mode %d)", i, pl->mode, MCSAS_EXEC_WAVE);
        if (pl->trace_capacity > 0)
            return fail(MCSAS_EINVAL, "launch_batch: plan %d has a trace (mcsas_hip_plan_set_trace, capacity %d); a batch records none: clear it, or launch the plan alone", i, (int)pl->trace_capacity);
        if (pl->dev != plans[0]->dev) return fail(MCSAS_EINVAL, "launch_batch: plan %d is on device %d, plan 0 on device %d", i, pl->dev, plans[0]->dev);
        if (pl->prob.stop != plans[0]->prob.stop) return fail(MCSAS_EINVAL, "launch_batch: plan %d has another stop word than plan 0 (all plans of a batch share one, or none has one)", i);
        for (int j = 0; j < i; ++j)
            if (plans[j] == pl) return fail(MCSAS_EINVAL, "launch_batch: plan %d is plan %d again", i, j);
    }
    DeviceGuard dev_guard;
    HIPCHK(hipSetDevice(plans[0]->dev));
    hipStream_t st = (hipStream_t)hip_stream;
    // the kernel of every plan; groups in order of first appearance
    std::vector<int> group_of(n);
    std::vector<KernelRef> groups;
    for (int i = 0; i < n; ++i) {
        KernelRef k;
        if (int rc = launch_kernel_of(plans[i], true, &k)) return rc;
        group_of[i] = (int)(std::find_if(groups.begin(), groups.end(), [&](const KernelRef &g) { return g.id() == k.id(); }) - groups.begin());
        if (group_of[i] == (int)groups.size()) groups.push_back(k);
    }
    // every plan's earlier analyses must be over before its workspaces are written again (as mcsas_hip_plan_launch_slot)
    for (int i = 0; i < n; ++i) {
        mcsas_plan *pl = plans[i];
        if (int rc = plan_activate_slot(pl, 0)) return rc;
        for (int k = 1; k < MCSAS_PLAN_SLOTS; ++k)
            if (pl->slots[k].launched && pl->slots[k].ev1) HIPCHK(hipStreamWaitEvent(st, pl->slots[k].ev1, 0));
        if (pl->cur().launched && pl->cur().ev1) HIPCHK(hipEventSynchronize(pl->cur().ev1));
    }
    // the shared block: relay, argument blocks, chain table (group-major, plans in list order, repetitions in order)
    size_t n_chains = 0;
    for (int i = 0; i < n; ++i) n_chains += (size_t)plans[i]->prob.n_reps;
    if (n_chains > 0x7fffffffull) return fail(MCSAS_EINVAL, "launch_batch: %zu chains", n_chains);
    const size_t off_sets = 256, off_chains = off_sets + (sizeof(ChainArgs) * (size_t)n + 255) / 256 * 256;
    auto bs = std::make_shared<BatchShared>();
    bs->dev = plans[0]->dev;
    bs->bytes = off_chains + sizeof(ChainRef) * n_chains;
    HIPCHK(cached_dev_malloc((void **)&bs->d_block, bs->bytes));
    HIPCHK(cached_host_malloc((void **)&bs->h_block, bs->bytes, hipHostMallocDefault));
    HIPCHK(bs->stop.make());
    const volatile int32_t *stop = plans[0]->prob.stop;
    *bs->stop.h = (stop && *stop) ? 1 : 0;
    // the relay starts as the stop word is now: a stop set before the launch is seen by every chain at its first poll (through the
    // host word alone only the chain that reads it would, the others one poll later)
    memset(bs->h_block, 0, off_sets);
    ((int32_t *)bs->h_block)[0] = *bs->stop.h;
    ChainArgs *h_sets = (ChainArgs *)(bs->h_block + off_sets);
    ChainRef *h_chains = (ChainRef *)(bs->h_block + off_chains);
    for (int i = 0; i < n; ++i) {
        h_sets[i] = plans[i]->args;                                          // (slot 0's outputs, the plan's seed / rep_offset)
        h_sets[i].stop_flag = bs->stop.d;
        h_sets[i].stop_relay = (int32_t *)bs->d_block;
    }
    std::vector<size_t> g_first(groups.size() + 1, 0), g_lds(groups.size(), 0);
    for (int i = 0; i < n; ++i) {
        g_first[group_of[i] + 1] += (size_t)plans[i]->prob.n_reps;
        g_lds[group_of[i]] = std::max(g_lds[group_of[i]], plans[i]->lds_bytes);
    }
    for (size_t g = 0; g < groups.size(); ++g) g_first[g + 1] += g_first[g];
    {
        std::vector<size_t> fill(g_first.begin(), g_first.end() - 1);
        for (int i = 0; i < n; ++i)
            for (int r = 0; r < plans[i]->prob.n_reps; ++r) h_chains[fill[group_of[i]]++] = ChainRef{i, r};
    }
    FailGuard guard{plans, n};                            // (an error return below may leave work on `st` that no end event covers)
    for (int i = 0; i < n; ++i) { plans[i]->stream = st; plans[i]->slots[0].batch_of = bs; }
    HIPCHK(hipMemcpyAsync(bs->d_block, bs->h_block, bs->bytes, hipMemcpyHostToDevice, st));
    for (int i = 0; i < n; ++i)
        if (plans[i]->has_start) { if (int rc = enqueue_start(plans[i], st)) return rc; }
    const ChainArgs *d_sets = (const ChainArgs *)(bs->d_block + off_sets);
    for (size_t g = 0; g < groups.size(); ++g) {
        const ChainRef *d_chains = (const ChainRef *)(bs->d_block + off_chains) + g_first[g];
        const unsigned grid = (unsigned)(g_first[g + 1] - g_first[g]);
        void *kargs[] = {(void *)&d_sets, (void *)&d_chains};
        for (int i = 0; i < n; ++i) if (group_of[i] == (int)g) HIPCHK(hipEventRecord(plans[i]->cur().ev0, st));
        if (int rc = raise_lds_limit(groups[g], g_lds[g])) return rc;
        if (int rc = launch_kernel(groups[g], grid, kargs, g_lds[g], st)) return rc;
        for (int i = 0; i < n; ++i)
            if (group_of[i] == (int)g) { HIPCHK(hipEventRecord(plans[i]->cur().ev1, st)); plans[i]->cur().launched = true; plans[i]->cur().traced = false; }
    }
    guard.ok = true;
    return MCSAS_OK;
}

// streams for hosts without a HIP binding of their own (ctypes / cgo callers that want analyses on several streams)
extern "C" int mcsas_hip_stream_create(int32_t device, void **stream) {
    if (!stream) return fail(MCSAS_EINVAL, "null argument");
    DeviceGuard dev_guard;
    int rc = select_device(device);
    if (rc) return rc;
    hipStream_t st = nullptr;
    HIPCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    *stream = (void *)st;
    return MCSAS_OK;
}
extern "C" void mcsas_hip_stream_destroy(void *stream) {
    if (stream) (void)hipStreamDestroy((hipStream_t)stream);
}

extern "C" int mcsas_hip_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}
extern "C" int mcsas_hip_abi_version(void) { return MCSAS_ABI_VERSION; }
extern "C" int mcsas_hip_is_tuning_build(void) {
#ifdef MCSAS_TUNING
    return 1;
#else
    return 0;
#endif
}
extern "C" const char *mcsas_hip_last_error(void) { return g_err.c_str(); }
