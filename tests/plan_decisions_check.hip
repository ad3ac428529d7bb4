// plan_decisions_check.hip — what the library decides without a device (csrc/host_decide.hip), as a stand-alone host program:
// tests/test_plan_decisions_host.py compiles this file together with host_decide.hip under AddressSanitizer and
// UndefinedBehaviorSanitizer and runs it.  No GPU: nothing in here or in that unit calls the HIP runtime.
//   plan_decisions_check                 the family table, the trace block's layout and transposition, the tick budget; prints "ok"
//   plan_decisions_check shapes < cases  one line per problem: what plan creation decides for it on a 256-CU device with nothing
//                                        ruled out by memory, or its refusal
//   plan_decisions_check gate < case     the free-memory gate of MCSAS_EXEC_AUTO on one problem; prints "ok" and the figures
// A problem is a line of text: id model_id nq n_contrib n_reps exec_mode waves_per_chain smear_nk n_active, the active indices,
// the MCSAS_MAX_PARAMS parameters.
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "host_decide.h"

using namespace mcsas;

// this program knows no plug-in
bool plugin_declares(int, int *, bool *) { return false; }

#define CHECK(cond)                                                                    \
    do {                                                                               \
        if (!(cond)) { fprintf(stderr, "%s:%d: CHECK(%s) failed; last error: %s\n", __FILE__, __LINE__, #cond, g_err.c_str()); exit(1); } \
    } while (0)

// ------------------------------------------------------------------------------ problems as text
struct TextProblem {
    char id[64];
    mcsas_problem p;
    std::vector<double> zeros;          // q, intensity, sigma and the smearing tables: their values do not enter the decision
};
static bool read_problem(TextProblem *t) {
    mcsas_problem &p = t->p;
    memset(&p, 0, sizeof p);
    if (scanf("%63s %d %d %d %d %d %d %d %d", t->id, &p.model_id, &p.nq, &p.n_contrib, &p.n_reps, &p.exec_mode, &p.waves_per_chain, &p.smear_nk, &p.n_active) != 9) return false;
    CHECK(p.n_active >= 0 && p.n_active <= MCSAS_MAX_ACTIVE && p.nq >= 1 && p.smear_nk >= 0);
    for (int c = 0; c < p.n_active; ++c) CHECK(scanf("%d", &p.active_index[c]) == 1);
    for (int i = 0; i < MCSAS_MAX_PARAMS; ++i) CHECK(scanf("%lf", &p.params[i]) == 1);
    p.struct_size = sizeof p;
    t->zeros.assign((size_t)p.nq * (size_t)(p.smear_nk > 0 ? p.smear_nk : 1), 0.);
    p.q = p.intensity = p.sigma = t->zeros.data();
    if (p.smear_nk > 0) p.smear_locs = p.smear_q_offset = p.smear_weights = t->zeros.data();
    p.max_iter = 100; p.cache_intensities = -1; p.device = -1;
    return true;
}
// validate_problem, fill_model_args and decide_shape, as mcsas_hip_plan_create calls them
static int decide(const mcsas_problem &p, size_t free_bytes, PlanShape *s) {
    if (int rc = validate_problem(&p)) return rc;
    ModelArgs margs;
    if (int rc = fill_model_args(&p, &margs)) return rc;
    return decide_shape(&p, margs, 256, free_bytes, tune_word(&p), s);
}

static int shapes() {
    TextProblem t;
    while (read_problem(&t)) {
        PlanShape s;
        if (const int rc = decide(t.p, SIZE_MAX, &s)) { printf("%s error %d %s\n", t.id, rc, g_err.c_str()); continue; }
        // (the window as mcsas_hip_plan_info reports it)
        const int window = s.mode == MCSAS_EXEC_PIPELINE ? s.pipe.kb : (s.mode == MCSAS_EXEC_WORKGROUP && !s.wide ? s.wg.window : 1);
        printf("%s shape %d %d %d %d\n", t.id, s.mode, s.waves, s.qpl, window);
    }
    return 0;
}

// The documented rule, restated: the pipeline needs R ((N + 2 Kb + 1) 8 qpad + 2 Kb (8 qpad + 8 (w + 4 + 4) + 4)) bytes — its row
// cache and its window buffers — and MCSAS_EXEC_AUTO drops it when that is at least half of what is free.
static int gate() {
    TextProblem t;
    CHECK(read_problem(&t));
    PlanShape s;
    CHECK(decide(t.p, SIZE_MAX, &s) == MCSAS_OK && s.mode == MCSAS_EXEC_PIPELINE);
    const unsigned long long R = t.p.n_reps, N = t.p.n_contrib, Kb = s.pipe.kb, w = s.pipe.w, qpad = s.qpad;
    const unsigned long long need = R * ((N + 2 * Kb + 1) * 8 * qpad + 2 * Kb * (8 * qpad + 8 * (w + 4 + 4) + 4));
    PlanShape g;
    CHECK(decide(t.p, (size_t)(2 * need + 2), &g) == MCSAS_OK && g.mode == MCSAS_EXEC_PIPELINE);      // just above twice the need
    CHECK(decide(t.p, (size_t)(2 * need), &g) == MCSAS_OK && g.mode != MCSAS_EXEC_PIPELINE);          // exactly half of what is free
    CHECK(decide(t.p, (size_t)(2 * need - 2), &g) == MCSAS_OK && g.mode != MCSAS_EXEC_PIPELINE);      // just below
    CHECK(decide(t.p, (size_t)288 << 30, &g) == MCSAS_OK && g.mode == MCSAS_EXEC_WAVE && g.waves == 1);   // an MI355X's 288 GiB
    printf("ok need %llu kb %llu w %llu qpad %llu\n", need, Kb, w, qpad);
    return 0;
}

// ------------------------------------------------------------------------------ the family table
// what resolve_kernel gave before the table, by hand; block sizes for a plan of 5 waves per chain
static void family_table() {
    static const struct { KernelFamily family; const char *word; unsigned block; FamilyInfo::Arg2 arg2; bool trace; } want[] = {
        {KF_WAVE, "", 64, FamilyInfo::ARG2_NONE, false},          {KF_WAVE_BATCH, "batch ", 64, FamilyInfo::ARG2_NONE, false},
        {KF_WG, "", 320, FamilyInfo::ARG2_WG, false},             {KF_WIDE, "q-split ", 320, FamilyInfo::ARG2_Q3INV, false},
        {KF_PIPE_TICK, "pipeline ", 512, FamilyInfo::ARG2_NONE, false}, {KF_WAVE_TRACE, "traced ", 64, FamilyInfo::ARG2_NONE, true},
        {KF_WIDE_TRACE, "traced q-split ", 320, FamilyInfo::ARG2_Q3INV, true}};
    static_assert(sizeof want / sizeof want[0] == KF_COUNT, "a row per family");
    for (const auto &x : want) {
        const FamilyInfo &f = KERNEL_FAMILY[x.family];
        CHECK(!strcmp(f.word, x.word) && family_block(x.family, 5) == x.block && f.arg2 == x.arg2 && f.trace == x.trace);
    }
    // a plug-in's instances: name expression and program key, cold and started
    static const struct { KernelFamily family; int qpl; bool flag, given; const char *expr, *key; } names[] = {
        {KF_WAVE, 8, true, false, "mcsas::chain_wave_kernel<MCSAS_MODEL_PLUGIN, 8, true, false>", "wave 8 1"},
        {KF_WAVE, 2, false, true, "mcsas::chain_wave_kernel<MCSAS_MODEL_PLUGIN, 2, false, true>", "wave start 2 0"},
        {KF_WAVE_BATCH, 4, true, false, "mcsas::chain_wave_batch_kernel<MCSAS_MODEL_PLUGIN, 4, true, false>", "wave batch 4 1"},
        {KF_WAVE_BATCH, 4, false, true, "mcsas::chain_wave_batch_kernel<MCSAS_MODEL_PLUGIN, 4, false, true>", "wave batch start 4 0"},
        {KF_WG, 2, true, false, "mcsas::chain_wg_kernel<MCSAS_MODEL_PLUGIN, 2>", "wg 2"},
        {KF_WIDE, 16, false, false, "mcsas::chain_wide_kernel<MCSAS_MODEL_PLUGIN, 16, false>", "wide 16"},
        {KF_WIDE, 32, true, true, "mcsas::chain_wide_kernel<MCSAS_MODEL_PLUGIN, 32, true>", "wide start 32"},
        {KF_PIPE_TICK, 2, true, false, "mcsas::pipe_tick_kernel<MCSAS_MODEL_PLUGIN, 2, true>", "pipe 2 1"},
        {KF_PIPE_TICK, 16, false, false, "mcsas::pipe_tick_kernel<MCSAS_MODEL_PLUGIN, 16, false>", "pipe 16 0"},
        {KF_WAVE_TRACE, 1, true, false, "mcsas::chain_wave_trace_kernel<MCSAS_MODEL_PLUGIN, 1, true, false>", "wave trace 1 1"},
        {KF_WAVE_TRACE, 64, false, true, "mcsas::chain_wave_trace_kernel<MCSAS_MODEL_PLUGIN, 64, false, true>", "wave trace start 64 0"},
        {KF_WIDE_TRACE, 8, false, false, "mcsas::chain_wide_trace_kernel<MCSAS_MODEL_PLUGIN, 8, false>", "wide trace 8"},
        {KF_WIDE_TRACE, 8, false, true, "mcsas::chain_wide_trace_kernel<MCSAS_MODEL_PLUGIN, 8, true>", "wide trace start 8"}};
    for (const auto &x : names) {
        std::string expr, key;
        CHECK(plugin_kernel_name(MCSAS_MODEL_PLUGIN0, x.family, x.qpl, x.flag, x.given, &expr, &key) == MCSAS_OK);
        if (expr != x.expr || key != x.key) { fprintf(stderr, "family %d: \"%s\" / \"%s\"\n", (int)x.family, expr.c_str(), key.c_str()); exit(1); }
    }
    // the families without a start refuse a given set
    std::string expr, key;
    char msg[96];
    CHECK(plugin_kernel_name(MCSAS_MODEL_PLUGIN0 + 1, KF_WG, 4, false, true, &expr, &key) == MCSAS_EINVAL);
    snprintf(msg, sizeof msg, "no wg start kernel for model %d qpl 4", MCSAS_MODEL_PLUGIN0 + 1);
    CHECK(g_err == msg);
    CHECK(plugin_kernel_name(MCSAS_MODEL_PLUGIN0, KF_PIPE_TICK, 2, true, true, &expr, &key) == MCSAS_EINVAL);
    snprintf(msg, sizeof msg, "no pipe start kernel for model %d qpl 2", MCSAS_MODEL_PLUGIN0);
    CHECK(g_err == msg && expr.empty() && key.empty());
}

// ------------------------------------------------------------------------------ the trace block and the tick budget
static void trace_block() {
    const size_t R = 3, K = 5, P = 2;
    constexpr TraceLayout at(3, 5, 2);
    static_assert(at.move_bytes == 32 && at.step == 0 && at.chisq == 120 && at.values == 240 && at.chisq0 == 480, "offsets");
    static_assert(at.host_bytes == 504 && at.dev_bytes == 512, "sizes");
    static_assert(TraceLayout(1, 1, 4).move_bytes == 48 && TraceLayout(7, 0, 1).dev_bytes == 256, "sizes");
    // 2 GiB: 1024 repetitions of 32 bytes per move hold 65536 moves each and not one more
    static_assert(!TraceLayout::too_large(1024, 65536, 2) && TraceLayout::too_large(1024, 65537, 2), "TRACE_MAX_BYTES");
    // a block as the kernels leave it, [rep][move]: step 100 r + i, chisq r + i / 8, values 1000 r + 10 i + p, chisq0 -r
    std::vector<char> block(at.host_bytes);
    int64_t *step = (int64_t *)(block.data() + at.step);
    double *chisq = (double *)(block.data() + at.chisq), *values = (double *)(block.data() + at.values), *chisq0 = (double *)(block.data() + at.chisq0);
    for (size_t r = 0; r < R; ++r) {
        chisq0[r] = -(double)r;
        for (size_t i = 0; i < K; ++i) {
            step[r * K + i] = (int64_t)(100 * r + i); chisq[r * K + i] = (double)r + (double)i / 8.;
            for (size_t p = 0; p < P; ++p) values[(r * K + i) * P + p] = (double)(1000 * r + 10 * i + p);
        }
    }
    ChainOut out[3] = {};
    const int64_t moves[3] = {0, 2, 7};                    // none, some, more than the block holds
    for (size_t r = 0; r < R; ++r) out[r].num_moves = moves[r];
    std::vector<int64_t> count(R), tstep(K * R);           // (exact sizes: the sanitizer sees a write past any of them)
    std::vector<double> tchi0(R), tchi(K * R), tval(K * P * R);
    mcsas_trace tr;
    memset(&tr, 0, sizeof tr);
    tr.struct_size = sizeof tr; tr.capacity = (int32_t)K;
    tr.count = count.data(); tr.chisq0 = tchi0.data(); tr.step = tstep.data(); tr.chisq = tchi.data(); tr.values = tval.data();
    CHECK(check_trace_arrays("check", &tr) == MCSAS_OK);
    trace_transpose(block.data(), R, K, P, out, &tr);
    for (size_t r = 0; r < R; ++r) {
        CHECK(count[r] == moves[r] && tchi0[r] == -(double)r);
        for (size_t i = 0; i < K; ++i) {
            const bool kept = (int64_t)i < moves[r];
            CHECK(tstep[i * R + r] == (kept ? (int64_t)(100 * r + i) : -1));
            CHECK(kept ? tchi[i * R + r] == (double)r + (double)i / 8. : std::isnan(tchi[i * R + r]));
            for (size_t p = 0; p < P; ++p)
                CHECK(kept ? tval[(i * P + p) * R + r] == (double)(1000 * r + 10 * i + p) : std::isnan(tval[(i * P + p) * R + r]));
        }
    }
}

static void tick_budget() {
    CHECK(pipeline_tick_budget(20000, 0, 192) == 106);                       // ceil(20000 / 192) + 1
    const int64_t huge = (int64_t)1 << 62;
    for (int32_t retries : {0, 1, 5, INT32_MAX}) CHECK(pipeline_tick_budget(huge, retries, 192) == 2000000000LL);
    CHECK(pipeline_tick_budget(huge, 0, 1) == 2000000000LL && pipeline_tick_budget(huge, 5, 1) == 2000000000LL);
    CHECK(pipeline_tick_budget(0, 0, 192) == 1 && pipeline_tick_budget(0, 2, 192) == 16);         // (0 + 191) / 192 + 1; 3 (0 + 4) + 4
    CHECK(pipeline_tick_budget(100, 0, 192) == 2 && pipeline_tick_budget(100, 5, 192) == 28);     // 291 / 192 + 1; 6 (0 + 4) + 4
    CHECK(pipeline_tick_budget(20000, 5, 192) == 652);                       // 6 (104 + 4) + 4
}

int main(int argc, char **argv) {
    if (argc > 1 && !strcmp(argv[1], "shapes")) return shapes();
    if (argc > 1 && !strcmp(argv[1], "gate")) return gate();
    family_table();
    trace_block();
    tick_budget();
    printf("ok\n");
    return 0;
}
