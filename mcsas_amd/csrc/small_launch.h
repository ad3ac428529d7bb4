// small_launch.h — from a model id to the instance of a small model kernel (small_kernels.h), said once for host_calls.hip and
// host_hist.hip.  Host code only: the run-time compiler never sees this file.
#pragma once
#include "host_internal.h"
#include "small_kernels.h"
#include "model_list.h"      // MCSAS_FOR_MODELS: the built-in models

// A family of small kernels: the template's instance for a built-in model, and which of a plug-in's small kernels stands for it
// (host_plugin.hip: PLUGIN_SMALL_EXPRS) — or none: hist_rows_batch_kernel has no plug-in form.
struct ModelRowsFamily {
    template <int M> static constexpr auto kernel = mcsas::model_rows_kernel<M>;
    static constexpr int plugin = PLUGIN_MODEL_ROWS;
};
struct ObservabilityFamily {
    template <int M> static constexpr auto kernel = mcsas::observability_kernel<M>;
    static constexpr int plugin = PLUGIN_OBSERVABILITY;
};
struct HistRowsFamily {
    template <int M> static constexpr auto kernel = mcsas::hist_rows_kernel<M>;
    static constexpr int plugin = PLUGIN_HIST_ROWS;
};
struct HistRowsBatchFamily {
    template <int M> static constexpr auto kernel = mcsas::hist_rows_batch_kernel<M>;
    static constexpr int plugin = -1;
};

// T, where a function parameter must not take part in deducing it
template <class T> struct as_declared { typedef T type; };

// launch_small_kernel with the kernel's parameter types P spelt out: whatever the caller passed has become a P by the time it is
// handed on — to a built-in instance by value, to a plug-in's kernel by address, where a value of another size would be read wrong.
template <class F, class... P>
static int launch_small_kernel_as(void (*)(P...), int model_id, dim3 grid, size_t lds, typename as_declared<P>::type... args) {
    switch (model_id) {
#define CASE_K(mm) case mm: F::template kernel<mm><<<grid, mcsas::WAVE, lds>>>(args...); break;
        MCSAS_FOR_MODELS(CASE_K)
#undef CASE_K
        default:
            if (F::plugin < 0) return fail(MCSAS_EINVAL, "model %d has no batch kernel", model_id);
            if (!is_plugin_model(model_id)) return fail(MCSAS_EINVAL, "model %d", model_id);
            if (int rc = plugin_small_launch(model_id, (PluginSmallKernel)F::plugin, grid, lds, args...)) return rc;
    }
    HIPCHK(hipGetLastError());
    return MCSAS_OK;
}
// The kernel of family F for `model_id` on the null stream, one wave per block: the arguments are converted to the parameter types of
// the built-in instances, which are the plug-in instance's too (one template).
template <class F, class... A>
static int launch_small_kernel(int model_id, dim3 grid, size_t lds, A... args) {
    return launch_small_kernel_as<F>(F::template kernel<MCSAS_MODEL_SPHERE>, model_id, grid, lds, args...);
}
