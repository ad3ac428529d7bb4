// host_sets.hip — mcsas_hip_analyse_sets and mcsas_hip_analyse_sets_mode: one population fitted to several data sets, each with a
// background of its own and a scale of its own or one for all (include/mcsas_hip.h; the kernels: chain_sets.h, instantiated per model
// in kern_wave_sets.hip and kern_wave_sets_shared.hip).  A one-shot call without a plan, and of
// it what needs a device: what the call refuses, where the sets lie (each padded to whole register slots of 64 entries) and the padded
// data are host_decide.hip's; here the kernel is looked up, one wavefront per repetition launched on the null stream and the results
// placed through host_result.h.
#include <hip/hip_runtime.h>

#include <vector>

#include "host_decide.h"    // check_sets_request, lay_out_sets; of chain_sets.h SetsArgs and SetsOut, the kernel template is not instantiated here
#include "host_result.h"
#include "model_list.h"

using namespace mcsas;

// the lookups of the built-in models (kern_wave_sets.hip, kern_wave_sets_shared.hip: `void *(int qpl, bool)`, the flag is not read),
// one row per scale mode
typedef void *SetsLookup(int qpl, bool flag);
#define DECL_SETS(m) SetsLookup mcsas_wave_sets_kernel_m##m, mcsas_wave_sets_shared_kernel_m##m;
#define ROW_SETS(m) mcsas_wave_sets_kernel_m##m,
#define ROW_SETS_SHARED(m) mcsas_wave_sets_shared_kernel_m##m,
MCSAS_FOR_MODELS(DECL_SETS)
static SetsLookup *const SETS_KERNEL[2][MCSAS_MODEL_COUNT] = {{MCSAS_FOR_MODELS(ROW_SETS)}, {MCSAS_FOR_MODELS(ROW_SETS_SHARED)}};
static_assert(MCSAS_SETS_SCALE_PER_SET == 0 && MCSAS_SETS_SCALE_SHARED == 1, "SETS_KERNEL's rows");
#undef DECL_SETS
#undef ROW_SETS
#undef ROW_SETS_SHARED

static int run_sets(const mcsas_problem *p, const SetsLayout &L, const ModelArgs &margs, mcsas_result *res, mcsas_sets_result *sets) {
    DeviceGuard guard;
    if (int rc = select_device(p->device)) return rc;
    const size_t R = p->n_reps, N = p->n_contrib, P = p->n_active, qpad = (size_t)L.qpl * WAVE;
    const int S = L.S;
    ChainArgs a;
    memset(&a, 0, sizeof a);
    SetsArgs sa;
    SetsData h;
    lay_out_sets(p, L, &h, &sa);

    DevBuf<double> dq, dw, dwI, dI, drset, dcache, dfit, dreplay;
    DevBuf<ChainOut> dout;
    DevBuf<SetsOut> dsout;
    DevBuf<int32_t> drelay;
    const size_t cache_rows = N + ((N & 1) ? 0 : 1);                            // an odd number of rows per chain (mcsas_hip.hip: alloc_rows)
    HIPCHK(dq.alloc(qpad)); HIPCHK(dw.alloc(qpad)); HIPCHK(dwI.alloc(qpad)); HIPCHK(dI.alloc(qpad));
    HIPCHK(drset.alloc(R * N * P)); HIPCHK(dcache.alloc(R * cache_rows * qpad)); HIPCHK(dfit.alloc(R * qpad));
    HIPCHK(dout.alloc(R)); HIPCHK(dsout.alloc(R)); HIPCHK(drelay.alloc(4));
    const size_t vb = sizeof(double) * qpad;
    HIPCHK(hipMemcpy(dq.p, h.q.data(), vb, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dw.p, h.w.data(), vb, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dwI.p, h.wI.data(), vb, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dI.p, h.I.data(), vb, hipMemcpyHostToDevice));
    if (p->replay_stream) {
        HIPCHK(dreplay.alloc(R * (size_t)p->replay_len));
        HIPCHK(copy_replay(dreplay.p, p, R));
    }
    StopWord stop;
    HIPCHK(stop.make());
    *stop.h = (p->stop && *p->stop) ? 1 : 0;
    // the relay starts as the stop word is now, as a batch's does (mcsas_hip.hip): a stop set before the call is seen by every chain at
    // its first poll (through the host word alone only the chain that reads it would, the others 64 steps later)
    const int32_t relay[4] = {*stop.h, 0, 0, 0};
    HIPCHK(hipMemcpy(drelay.p, relay, sizeof relay, hipMemcpyHostToDevice));

    a.model = margs;
    a.nq = p->nq; a.qpad = (int)qpad;
    a.q = dq.p; a.w = dw.p; a.wI = dwI.p; a.I = dI.p;
    fill_chain_settings(p, &a);
    a.pos_bg = 0;                                                               // (refused when asked for)
    a.replay = dreplay.p; a.replay_len = p->replay_stream ? p->replay_len : 0;
    a.stop_flag = stop.d; a.stop_relay = drelay.p;
    a.rset = drset.p; a.cache = dcache.p; a.cache_rows = (int)cache_rows; a.fit = dfit.p; a.out = dout.p;
    sa.out = dsout.p;

    void *const kernel = SETS_KERNEL[sa.scale_mode][p->model_id](L.qpl, true);
    if (L.lds_bytes > 64 * 1024) HIPCHK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)L.lds_bytes));
    void *kargs[2] = {(void *)&a, (void *)&sa};
    HIPCHK(hipLaunchKernel(kernel, dim3((unsigned)R), dim3(WAVE), kargs, L.lds_bytes, nullptr));
    // wait, forwarding the caller's stop word to the device-visible one (McSAS.stop, mcsas.py:357)
    if (p->stop) {
        hipEvent_t done;
        HIPCHK(hipEventCreateWithFlags(&done, hipEventDisableTiming));
        const hipError_t e = hipEventRecord(done, nullptr);
        const int rc = e == hipSuccess ? wait_forwarding_stop("analyse_sets: ", done, p->stop, stop.h)
                                       : fail(MCSAS_EHIP, "analyse_sets: kernel failed: %s", hipGetErrorString(e));
        (void)hipEventDestroy(done);
        if (rc) return rc;
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

extern "C" int mcsas_hip_analyse_sets_mode(const mcsas_problem *p, int32_t n_sets, const int32_t *set_nq, int32_t scale_mode, mcsas_result *res,
                                           mcsas_sets_result *sets) {
    SetsLayout L;
    ModelArgs margs;
    if (int rc = check_sets_request(p, n_sets, set_nq, res, sets, &L, &margs, scale_mode)) return rc;
    if (!SETS_KERNEL[scale_mode][p->model_id](L.qpl, true)) return fail(MCSAS_EINVAL, "analyse_sets: no kernel for model %d qpl %d", p->model_id, L.qpl);
    return no_bad_alloc("analyse_sets", [&] { return run_sets(p, L, margs, res, sets); });
}
extern "C" int mcsas_hip_analyse_sets(const mcsas_problem *p, int32_t n_sets, const int32_t *set_nq, mcsas_result *res,
                                      mcsas_sets_result *sets) {
    return mcsas_hip_analyse_sets_mode(p, n_sets, set_nq, MCSAS_SETS_SCALE_PER_SET, res, sets);
}
