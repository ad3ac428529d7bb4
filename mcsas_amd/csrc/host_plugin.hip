// host_plugin.hip — run-time model plug-ins (hiprtc) of libmcsas_hip.so.
// The reference takes any models/*.py that subclasses ScatteringModel (utils/findmodels.py:120-186); here a model outside
// the eight built-in ones arrives as HIP source text defining the four functions of plugin_model.h.  It is compiled for gfx950
// against the library's OWN kernel headers (embedded at build time: embedded_headers.inc) — the chain kernels and the
// three model-templated small kernels, instantiated for Contrib<MCSAS_MODEL_PLUGIN> — and loaded as a code-object module on
// every device that uses it.  Compilation needs no GPU; loading does.
#include <hip/hip_runtime.h>
#include <hip/hiprtc.h>

#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "host_decide.h"
#include "embedded_headers.inc"

struct Plugin {
    std::string source;
    int row_class = 0;                  // `#define MCSAS_PLUGIN_ROW_CLASS n` in the text (plugin_model.h)
    bool can_smear = false;             // `#define MCSAS_PLUGIN_CAN_SMEAR 1`
    std::mutex mu;
    struct Program { std::vector<char> code; std::map<std::string, std::string> lowered; };
    std::map<std::string, Program> programs;                                  // by program key ("small", "wave 8 1", ...)
    std::map<std::pair<int, std::string>, hipModule_t> modules;               // (device, program key)
};
static std::mutex g_plugins_mu;
static std::vector<std::unique_ptr<Plugin>> g_plugins;
static thread_local std::string g_plugin_log;

static Plugin *plugin_of(int model_id) {
    std::lock_guard<std::mutex> lk(g_plugins_mu);
    const int k = model_id - MCSAS_MODEL_PLUGIN0;
    return (k >= 0 && k < (int)g_plugins.size()) ? g_plugins[k].get() : nullptr;
}
bool plugin_declares(int model_id, int *row_class, bool *can_smear) {
    const Plugin *pg = plugin_of(model_id);
    if (!pg) return false;
    if (row_class) *row_class = pg->row_class;
    if (can_smear) *can_smear = pg->can_smear;
    return true;
}

// one translation unit: the kernel headers, the plug-in's Contrib, the plug-in text; `exprs` = the kernels to instantiate
// value of the LAST `#define KEY value` line of the text (whitespace after '#' and around the name, parentheses around the
// value allowed), `dflt` when there is none.  What this returns is checked against the preprocessor (see mcsas_hip_plugin_compile).
static long plugin_scan_define(const std::string &src, const char *key, long dflt) {
    long val = dflt;
    const size_t klen = strlen(key);
    size_t pos = 0;
    while (pos < src.size()) {
        size_t eol = src.find('\n', pos);
        if (eol == std::string::npos) eol = src.size();
        size_t i = pos;
        auto skip_ws = [&]() { while (i < eol && (src[i] == ' ' || src[i] == '\t')) ++i; };
        skip_ws();
        if (i < eol && src[i] == '#') {
            ++i; skip_ws();
            if (src.compare(i, 6, "define") == 0) {
                i += 6;
                const size_t before = i;
                skip_ws();
                if (i > before && src.compare(i, klen, key) == 0 && (i + klen >= eol || src[i + klen] == ' ' || src[i + klen] == '\t')) {
                    i += klen; skip_ws();
                    while (i < eol && src[i] == '(') { ++i; skip_ws(); }
                    val = i < eol ? strtol(src.c_str() + i, nullptr, 0) : 1;     // `#define KEY` alone: defined, i.e. 1 where it is used as a flag
                }
            }
        }
        pos = eol + 1;
    }
    return val;
}

static int plugin_compile_program(const Plugin &pg, const std::vector<std::string> &exprs, Plugin::Program *out) {
    const std::string &source = pg.source;
    // hiprtc has the fixed-width integer types in a namespace of its own
    std::string tu =
        "typedef signed char int8_t; typedef unsigned char uint8_t; typedef short int16_t; typedef unsigned short uint16_t;\n"
        "typedef int int32_t; typedef unsigned int uint32_t; typedef long int64_t; typedef unsigned long uint64_t;\n"
        "#include \"chain_common.h\"\n#line 1 \"plugin\"\n";
    tu += source;
    tu += "\n#include \"plugin_model.h\"\n#include \"chain_wave.h\"\n#include \"chain_wg.h\"\n#include \"chain_wide.h\"\n#include \"chain_pipe.h\"\n#include \"small_kernels.h\"\n";
    hiprtcProgram prog = nullptr;
    hiprtcResult r = hiprtcCreateProgram(&prog, tu.c_str(), "mcsas_plugin.hip", mcsas_embedded_count, const_cast<const char **>(mcsas_embedded_texts),
                                         const_cast<const char **>(mcsas_embedded_names));
    if (r != HIPRTC_SUCCESS) return fail(MCSAS_EHIP, "hiprtcCreateProgram: %s", hiprtcGetErrorString(r));
    for (const std::string &e : exprs) hiprtcAddNameExpression(prog, e.c_str());
    // the flags of the Makefile: one contribution row must come out the same from every call site (-ffp-contract=off)
    char host_rc[48], host_cs[48];
    snprintf(host_rc, sizeof host_rc, "-DMCSAS_HOST_ROW_CLASS=%d", pg.row_class);
    snprintf(host_cs, sizeof host_cs, "-DMCSAS_HOST_CAN_SMEAR=%d", pg.can_smear ? 1 : 0);
    const char *opts[] = {"--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-Wno-unused-value", host_rc, host_cs};
    r = hiprtcCompileProgram(prog, (int)(sizeof opts / sizeof opts[0]), opts);
    size_t ls = 0;
    g_plugin_log.clear();
    if (hiprtcGetProgramLogSize(prog, &ls) == HIPRTC_SUCCESS && ls > 1) { g_plugin_log.resize(ls); hiprtcGetProgramLog(prog, &g_plugin_log[0]); }
    if (r != HIPRTC_SUCCESS) {
        hiprtcDestroyProgram(&prog);
        return fail(MCSAS_EINVAL, "model plug-in does not compile (%s): see mcsas_hip_plugin_log()", hiprtcGetErrorString(r));
    }
    size_t cs = 0;
    hiprtcGetCodeSize(prog, &cs);
    out->code.resize(cs);
    hiprtcGetCode(prog, out->code.data());
    for (const std::string &e : exprs) {
        const char *ln = nullptr;
        if (hiprtcGetLoweredName(prog, e.c_str(), &ln) != HIPRTC_SUCCESS || !ln) { hiprtcDestroyProgram(&prog); return fail(MCSAS_EHIP, "no lowered name for %s", e.c_str()); }
        out->lowered[e] = ln;
    }
    hiprtcDestroyProgram(&prog);
    return MCSAS_OK;
}

static const char *const PLUGIN_SMALL_EXPRS[3] = {"mcsas::model_rows_kernel<MCSAS_MODEL_PLUGIN>", "mcsas::observability_kernel<MCSAS_MODEL_PLUGIN>",
                                                  "mcsas::hist_rows_kernel<MCSAS_MODEL_PLUGIN>"};

// kernel `expr` of program `key` (compiled on first use) as a function of the CURRENT device's module
static int plugin_function(int model_id, const std::string &key, const std::vector<std::string> &exprs, const std::string &expr, hipFunction_t *fn) {
    Plugin *pg = plugin_of(model_id);
    if (!pg) return fail(MCSAS_EINVAL, "model_id %d: no such plug-in (mcsas_hip_plugin_compile returns the id)", model_id);
    std::lock_guard<std::mutex> lk(pg->mu);
    auto it = pg->programs.find(key);
    if (it == pg->programs.end()) {
        Plugin::Program prg;
        int rc = plugin_compile_program(*pg, exprs, &prg);
        if (rc) return rc;
        it = pg->programs.emplace(key, std::move(prg)).first;
    }
    int dev = 0;
    HIPCHK(hipGetDevice(&dev));
    auto mk = std::make_pair(dev, key);
    auto mi = pg->modules.find(mk);
    if (mi == pg->modules.end()) {
        hipModule_t mod = nullptr;
        HIPCHK(hipModuleLoadData(&mod, it->second.code.data()));
        mi = pg->modules.emplace(mk, mod).first;
    }
    HIPCHK(hipModuleGetFunction(fn, mi->second, it->second.lowered.at(expr).c_str()));
    return MCSAS_OK;
}
int plugin_small_function(int model_id, PluginSmallKernel which, hipFunction_t *fn) {
    const std::vector<std::string> exprs(PLUGIN_SMALL_EXPRS, PLUGIN_SMALL_EXPRS + 3);
    return plugin_function(model_id, "small", exprs, exprs[which], fn);
}
int plugin_chain_function(int model_id, KernelFamily family, int qpl, bool flag, bool given, hipFunction_t *fn) {
    std::string e, k;                                     // (KERNEL_FAMILY, host_internal.h: the template's name and arguments, the program key)
    if (int rc = plugin_kernel_name(model_id, family, qpl, flag, given, &e, &k)) return rc;
    return plugin_function(model_id, k, {e}, e, fn);
}

extern "C" int mcsas_hip_plugin_compile(const char *source, int32_t *model_id) {
    if (!source || !model_id) return fail(MCSAS_EINVAL, "null argument");
    *model_id = -1;
    {
        std::lock_guard<std::mutex> lk(g_plugins_mu);
        for (size_t k = 0; k < g_plugins.size(); ++k)
            if (g_plugins[k]->source == source) { *model_id = MCSAS_MODEL_PLUGIN0 + (int)k; return MCSAS_OK; }   // the same text again
    }
    // the small kernels are compiled here, so that a plug-in that does not compile is refused before anything uses it
    auto pg = std::make_unique<Plugin>();
    pg->source = source;
    // The row class and the canSmear flag the text declares: the host needs the numbers for the pipeline's geometry and for the
    // smearing tables, the kernels see the macros.  The host's reading of the text (a line-wise scan for `# define KEY value`)
    // is passed to EVERY compilation of this plug-in as -DMCSAS_HOST_ROW_CLASS / -DMCSAS_HOST_CAN_SMEAR and plugin_model.h
    // static_asserts that the preprocessor's values are the same: a text the scan misreads (a define inside a comment or an
    // `#if 0`, an expression for a value) does not compile and is refused here instead of running with two different answers.
    pg->row_class = (int)plugin_scan_define(pg->source, "MCSAS_PLUGIN_ROW_CLASS", 0);
    pg->can_smear = plugin_scan_define(pg->source, "MCSAS_PLUGIN_CAN_SMEAR", 0) != 0;
    if (pg->row_class < 0 || pg->row_class > 1) return fail(MCSAS_EINVAL, "MCSAS_PLUGIN_ROW_CLASS %d (0 or 1)", pg->row_class);
    Plugin::Program prg;
    const std::vector<std::string> exprs(PLUGIN_SMALL_EXPRS, PLUGIN_SMALL_EXPRS + 3);
    int rc = plugin_compile_program(*pg, exprs, &prg);
    if (rc) return rc;
    pg->programs.emplace("small", std::move(prg));
    std::lock_guard<std::mutex> lk(g_plugins_mu);
    if ((int)g_plugins.size() >= MCSAS_MAX_PLUGINS) return fail(MCSAS_EINVAL, "more than %d model plug-ins", MCSAS_MAX_PLUGINS);
    g_plugins.push_back(std::move(pg));
    *model_id = MCSAS_MODEL_PLUGIN0 + (int)g_plugins.size() - 1;
    return MCSAS_OK;
}
extern "C" const char *mcsas_hip_plugin_log(void) { return g_plugin_log.c_str(); }
