// host_sets.hip — mcsas_hip_analyse_sets: one population fitted to several data sets, each with a scale and a background of its own
// (include/mcsas_hip.h; the kernel: chain_sets.h, instantiated per model in kern_wave_sets.hip).  A one-shot call without a plan: what
// it refuses it refuses before a device is touched, then it lays the sets out for the kernel (each padded to whole register slots of 64
// entries), launches one wavefront per repetition on the null stream and places the results through host_result.h.
#include <hip/hip_runtime.h>

#include <chrono>
#include <new>
#include <thread>
#include <vector>

#include "host_decide.h"
#include "host_result.h"
#include "chain_sets.h"     // SetsArgs, SetsOut; the kernel template is not instantiated here
#include "model_list.h"

using namespace mcsas;

// the lookups of the built-in models (kern_wave_sets.hip: `void *(int qpl, bool)`, the flag is not read)
typedef void *SetsLookup(int qpl, bool flag);
#define DECL_SETS(m) SetsLookup mcsas_wave_sets_kernel_m##m;
#define ROW_SETS(m) mcsas_wave_sets_kernel_m##m,
MCSAS_FOR_MODELS(DECL_SETS)
static SetsLookup *const SETS_KERNEL[MCSAS_MODEL_COUNT] = {MCSAS_FOR_MODELS(ROW_SETS)};
#undef DECL_SETS
#undef ROW_SETS

constexpr int SETS_MAX_SLOTS = Q_MAX_WINDOW / WAVE;        // 16 register slots of 64 entries: the largest instance

// Where the sets lie in the padded vectors: set s at [pad_off[s], pad_off[s] + 64 slots[s]), its points at [off[s], off[s] + nq[s]) of
// the caller's; qpl is the smallest instantiated slot count that holds them all, bit j of end_mask marks a set's last slot.
struct SetsLayout {
    int S = 0, qpl = 0, total_slots = 0;
    int nq[MCSAS_MAX_SETS] = {}, off[MCSAS_MAX_SETS] = {}, slots[MCSAS_MAX_SETS] = {}, pad_off[MCSAS_MAX_SETS] = {};
    uint32_t end_mask = 0;
    size_t lds_bytes = 0;
};

// Everything the call refuses, in order, without a HIP call; fills the layout and the model's argument block.
static int check_sets_request(const mcsas_problem *p, int32_t n_sets, const int32_t *set_nq, const mcsas_result *res,
                              const mcsas_sets_result *sets, SetsLayout *L, ModelArgs *margs) {
    const char *const who = "analyse_sets";
    if (!p || !res || !sets || !set_nq) return fail(MCSAS_EINVAL, "%s: null argument", who);
    if (p->struct_size != sizeof(mcsas_problem))
        return fail(MCSAS_EINVAL, "%s: mcsas_problem size %u, library expects %zu (ABI mismatch)", who, p->struct_size, sizeof(mcsas_problem));
    if (res->struct_size != sizeof(mcsas_result)) return fail(MCSAS_EINVAL, "%s: mcsas_result size mismatch", who);
    if (sets->struct_size != sizeof(mcsas_sets_result))
        return fail(MCSAS_EINVAL, "%s: mcsas_sets_result size %u, library expects %zu", who, sets->struct_size, sizeof(mcsas_sets_result));
    if (n_sets < 1 || n_sets > MCSAS_MAX_SETS) return fail(MCSAS_EINVAL, "%s: n_sets %d (1..%d)", who, (int)n_sets, MCSAS_MAX_SETS);
    if (sets->n_sets != n_sets) return fail(MCSAS_EINVAL, "%s: mcsas_sets_result.n_sets %d, the call's n_sets is %d", who, (int)sets->n_sets, (int)n_sets);
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
    L->S = n_sets;
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
    if (!SETS_KERNEL[p->model_id](L->qpl, true)) return fail(MCSAS_EINVAL, "%s: no kernel for model %d qpl %d", who, p->model_id, L->qpl);
    return MCSAS_OK;
}

// the mapped host word the chains see McSAS.stop through (chain_common.h: stop_requested), back to the cache on the way out
struct StopWord {
    int32_t *h = nullptr;
    ~StopWord() { cached_host_free(h, sizeof(int32_t), hipHostMallocMapped); }
};

static int run_sets(const mcsas_problem *p, const SetsLayout &L, const ModelArgs &margs, mcsas_result *res, mcsas_sets_result *sets) {
    DeviceGuard guard;
    if (int rc = select_device(p->device)) return rc;
    const size_t R = p->n_reps, N = p->n_contrib, P = p->n_active, qpad = (size_t)L.qpl * WAVE;
    const int S = L.S;

    // the padded vectors (pad: q of the set's first point — behind the last set, of the first set's —, w = wI = I = 0; sigma == 0 -> 1,
    // backgroundscalingfit.py:117) and each set's sums, as WeighedData (host_internal.h) makes one set's
    ChainArgs a;
    memset(&a, 0, sizeof a);
    SetsArgs sa;
    memset(&sa, 0, sizeof sa);
    std::vector<double> hq(qpad, p->q[0]), hw(qpad, 0.), hwI(qpad, 0.), hI(qpad, 0.);
    for (int s = 0; s < S; ++s) {
        double Sw = 0, SI = 0, SII = 0;
        for (int i = 0; i < L.slots[s] * WAVE; ++i) hq[L.pad_off[s] + i] = p->q[L.off[s]];
        for (int i = 0; i < L.nq[s]; ++i) {
            const int src = L.off[s] + i, dst = L.pad_off[s] + i;
            const double e = p->sigma[src] == 0.0 ? 1.0 : p->sigma[src], wi = 1.0 / (e * e), I = p->intensity[src];
            hq[dst] = p->q[src]; hw[dst] = wi; hwI[dst] = wi * I; hI[dst] = I;
            Sw += wi; SI += wi * I; SII += wi * I * I;
        }
        // (1 / Sw, SI / Sw, SII - SI² / Sw: the operations of chain_body.inc, unfused here as there)
        sa.set[s] = SetConst{Sw, SI, SII, 1.0 / Sw, SI / Sw, SII - SI * SI / Sw, (double)L.nq[s]};
    }
    sa.n_sets = S; sa.end_mask = L.end_mask;

    DevBuf<double> dq, dw, dwI, dI, drset, dcache, dfit, dreplay;
    DevBuf<ChainOut> dout;
    DevBuf<SetsOut> dsout;
    DevBuf<int32_t> drelay;
    const size_t cache_rows = N + ((N & 1) ? 0 : 1);                            // an odd number of rows per chain (mcsas_hip.hip: alloc_rows)
    HIPCHK(dq.alloc(qpad)); HIPCHK(dw.alloc(qpad)); HIPCHK(dwI.alloc(qpad)); HIPCHK(dI.alloc(qpad));
    HIPCHK(drset.alloc(R * N * P)); HIPCHK(dcache.alloc(R * cache_rows * qpad)); HIPCHK(dfit.alloc(R * qpad));
    HIPCHK(dout.alloc(R)); HIPCHK(dsout.alloc(R)); HIPCHK(drelay.alloc(4));
    const size_t vb = sizeof(double) * qpad;
    HIPCHK(hipMemcpy(dq.p, hq.data(), vb, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dw.p, hw.data(), vb, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dwI.p, hwI.data(), vb, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dI.p, hI.data(), vb, hipMemcpyHostToDevice));
    HIPCHK(hipMemset(drelay.p, 0, 16));
    if (p->replay_stream) {
        HIPCHK(dreplay.alloc(R * (size_t)p->replay_len));
        HIPCHK(hipMemcpy(dreplay.p, p->replay_stream, sizeof(double) * R * (size_t)p->replay_len, hipMemcpyHostToDevice));
    }
    StopWord stop;
    HIPCHK(cached_host_malloc((void **)&stop.h, sizeof(int32_t), hipHostMallocMapped));
    *stop.h = (p->stop && *p->stop) ? 1 : 0;
    int32_t *d_stop = nullptr;
    HIPCHK(hipHostGetDevicePointer((void **)&d_stop, stop.h, 0));

    a.model = margs;
    a.nq = p->nq; a.qpad = (int)qpad;
    a.q = dq.p; a.w = dw.p; a.wI = dwI.p; a.I = dI.p;
    a.n_contrib = p->n_contrib; a.n_reps = p->n_reps;
    a.find_bg = p->find_background != 0; a.pos_bg = 0;
    a.start_from_min = p->start_from_minimum != 0; a.max_retries = p->max_retries;
    a.max_iter = p->max_iter; a.conv_crit = p->conv_crit;
    for (int c = 0; c < MCSAS_MAX_ACTIVE; ++c) {
        a.gen_lo[c] = p->gen_lo[c]; a.gen_hi[c] = p->gen_hi[c]; a.start_value[c] = p->start_value[c];
        a.gen_kind[c] = p->gen_kind[c];
    }
    a.seed = p->seed; a.rep_offset = p->rep_offset;
    a.replay = dreplay.p; a.replay_len = p->replay_stream ? p->replay_len : 0;
    a.stop_flag = d_stop; a.stop_relay = drelay.p;
    a.rset = drset.p; a.cache = dcache.p; a.cache_rows = (int)cache_rows; a.fit = dfit.p; a.out = dout.p;
    sa.out = dsout.p;

    void *const kernel = SETS_KERNEL[p->model_id](L.qpl, true);
    if (L.lds_bytes > 64 * 1024) HIPCHK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)L.lds_bytes));
    void *kargs[2] = {(void *)&a, (void *)&sa};
    HIPCHK(hipLaunchKernel(kernel, dim3((unsigned)R), dim3(WAVE), kargs, L.lds_bytes, nullptr));
    // wait, forwarding the caller's stop word to the device-visible one (McSAS.stop, mcsas.py:357)
    if (p->stop) {
        hipEvent_t done;
        HIPCHK(hipEventCreateWithFlags(&done, hipEventDisableTiming));
        hipError_t e = hipEventRecord(done, nullptr);
        while (e == hipSuccess && (e = hipEventQuery(done)) == hipErrorNotReady) {
            if (*(volatile const int32_t *)p->stop) *stop.h = 1;
            std::this_thread::sleep_for(std::chrono::microseconds(50));
            e = hipSuccess;
        }
        (void)hipEventDestroy(done);
        if (e != hipSuccess) return fail(MCSAS_EHIP, "analyse_sets: kernel failed: %s", hipGetErrorString(e));
    }
    HIPCHK(hipStreamSynchronize(nullptr));

    std::vector<ChainOut> ho(R);
    std::vector<SetsOut> hso(R);
    HIPCHK(hipMemcpy(ho.data(), dout.p, sizeof(ChainOut) * R, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(hso.data(), dsout.p, sizeof(SetsOut) * R, hipMemcpyDeviceToHost));
    if (res->contribs) {
        std::vector<double> hr(R * N * P);
        HIPCHK(hipMemcpy(hr.data(), drset.p, sizeof(double) * hr.size(), hipMemcpyDeviceToHost));
        result_put_sets(res, hr.data(), N, P, R, 0, R);
    }
    if (res->fit) {                                                            // un-padded: set s from its place in the padded rows
        std::vector<double> hf(R * qpad);
        HIPCHK(hipMemcpy(hf.data(), dfit.p, sizeof(double) * hf.size(), hipMemcpyDeviceToHost));
        for (int s = 0; s < S; ++s)
            result_put_block(res->fit + (size_t)L.off[s] * R, (size_t)L.nq[s], R, 0, R, (const double *)hf.data() + L.pad_off[s], 1, qpad);
    }
    int ovf = 0;
    for (size_t r = 0; r < R; ++r) {
        result_put_row(res, r, ho[r]);
        ovf |= ho[r].stream_overflow;
        for (int s = 0; s < S; ++s) {
            if (sets->scaling) sets->scaling[(size_t)s * R + r] = hso[r].scaling[s];
            if (sets->background) sets->background[(size_t)s * R + r] = hso[r].background[s];
            if (sets->chisq) sets->chisq[(size_t)s * R + r] = hso[r].chisq[s];
        }
    }
    if (ovf) return fail(MCSAS_ESTREAM, "replay stream exhausted (replay_len=%lld)", (long long)p->replay_len);
    return MCSAS_OK;
}

extern "C" int mcsas_hip_analyse_sets(const mcsas_problem *p, int32_t n_sets, const int32_t *set_nq, mcsas_result *res,
                                      mcsas_sets_result *sets) {
    SetsLayout L;
    ModelArgs margs;
    if (int rc = check_sets_request(p, n_sets, set_nq, res, sets, &L, &margs)) return rc;
    try {
        return run_sets(p, L, margs, res, sets);
    } catch (const std::bad_alloc &) {
        return fail(MCSAS_ENOMEM, "analyse_sets: out of host memory");
    }
}
