// plan_decisions_check.hip — what the library decides without a device (csrc/host_decide.hip), as a stand-alone host program:
// tests/test_plan_decisions_host.py compiles this file together with host_decide.hip under AddressSanitizer and
// UndefinedBehaviorSanitizer and runs it.  No GPU: nothing in here or in that unit calls the HIP runtime.
//   plan_decisions_check                 the family table, the trace block's layout and transposition, the tick budget, the settings
//                                        block of a chain run, the padded data and constants of several sets; prints "ok"
//   plan_decisions_check shapes < cases  one line per problem: what plan creation decides for it on a 256-CU device with nothing
//                                        ruled out by memory, or its refusal
//   plan_decisions_check gate < case     the free-memory gate of MCSAS_EXEC_AUTO on one problem; prints "ok" and the figures
//   plan_decisions_check sets < cases    one line per request of mcsas_hip_analyse_sets (id nq n_sets set_nq...): where the sets lie, or
//                                        the refusal
//   plan_decisions_check refusals < rows one line per request with one thing spoiled (id model_id n_active n_devices
//                                        positive_background smear_nk cache_intensities exec_mode): code and message
// A problem is a line of text: id model_id nq n_contrib n_reps exec_mode waves_per_chain smear_nk n_active, the active indices,
// the MCSAS_MAX_PARAMS parameters.
#include <cinttypes>
#include <cmath>
#include <cstddef>
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

// ------------------------------------------------------------------------------ the settings block of a chain run
static void chain_settings() {
    mcsas_problem p;
    memset(&p, 0, sizeof p);
    p.n_contrib = 11; p.n_reps = 12; p.find_background = 2; p.positive_background = 0; p.start_from_minimum = -1; p.max_retries = 13;
    p.max_iter = ((int64_t)1 << 40) + 14; p.conv_crit = 15.5; p.seed = 0x123456789abcdef0ull; p.rep_offset = 16; p.reserved0 = 17;
    for (int c = 0; c < MCSAS_MAX_ACTIVE; ++c) { p.gen_lo[c] = 20. + c; p.gen_hi[c] = 30. + c; p.start_value[c] = 40. + c; p.gen_kind[c] = c % 4; }
    ChainArgs a, untouched;
    memset((void *)&a, 0xA5, sizeof a); memset((void *)&untouched, 0xA5, sizeof untouched);
    fill_chain_settings(&p, &a);
    CHECK(a.find_bg == 1 && a.pos_bg == 0 && a.start_from_min == 1);
    CHECK(a.n_contrib == 11 && a.n_reps == 12 && a.max_retries == 13 && a.max_iter == p.max_iter && a.conv_crit == 15.5);
    CHECK(a.seed == p.seed && a.rep_offset == 16);
    for (int c = 0; c < MCSAS_MAX_ACTIVE; ++c)
        CHECK(a.gen_lo[c] == p.gen_lo[c] && a.gen_hi[c] == p.gen_hi[c] && a.start_value[c] == p.start_value[c] && a.gen_kind[c] == p.gen_kind[c]);
    // nothing else is written: the settings block [n_contrib, seed) and seed, rep_offset put back, the rest is as it was (pad0 too)
    memset((char *)&a + offsetof(ChainArgs, n_contrib), 0xA5, offsetof(ChainArgs, pad0) - offsetof(ChainArgs, n_contrib));
    CHECK(!memcmp((const void *)&a, (const void *)&untouched, sizeof a));
}

// ------------------------------------------------------------------------------ several sets fitted with one population
// A valid request over spheres: nq points with distinct q (1e7 (i + 1)), I = 5 + 0.37 i, sigma = 0.1 + 0.01 i; the caller breaks one thing.
struct SetsRequest {
    mcsas_problem p;
    mcsas_result res;
    mcsas_sets_result sets;
    std::vector<double> q, I, sig;
    std::vector<int32_t> set_nq;
    SetsLayout L;
    ModelArgs margs;
    SetsRequest(int nq, std::vector<int32_t> nqs) : q(nq), I(nq), sig(nq), set_nq(nqs) {
        memset(&p, 0, sizeof p); memset(&res, 0, sizeof res); memset(&sets, 0, sizeof sets);
        for (int i = 0; i < nq; ++i) { q[i] = 1e7 * (i + 1); I[i] = 5. + 0.37 * i; sig[i] = 0.1 + 0.01 * i; }
        p.struct_size = sizeof p; res.struct_size = sizeof res; sets.struct_size = sizeof sets; sets.n_sets = (int32_t)nqs.size();
        p.model_id = MCSAS_MODEL_SPHERE; p.nq = nq; p.q = q.data(); p.intensity = I.data(); p.sigma = sig.data();
        p.n_active = 1; p.params[0] = 1e-8; p.gen_lo[0] = 2e-9; p.gen_hi[0] = 3e-7; p.clip_hi[0] = 1.;
        p.n_contrib = 8; p.n_reps = 2; p.max_iter = 10; p.cache_intensities = -1; p.device = -1;
    }
    int check() { return check_sets_request(&p, (int32_t)set_nq.size(), set_nq.data(), &res, &sets, &L, &margs); }
};

static int sets_layouts() {
    char id[64];
    int nq, S;
    static_assert(SETS_LDS_DOUBLES == 40 && WAVE == 64, "the rule restated below");
    while (scanf("%63s %d %d", id, &nq, &S) == 3) {
        std::vector<int32_t> nqs(S);
        for (int s = 0; s < S; ++s) CHECK(scanf("%d", &nqs[s]) == 1);
        SetsRequest r(nq, nqs);
        if (const int rc = r.check()) { printf("%s error %d %s\n", id, rc, g_err.c_str()); continue; }
        const SetsLayout &L = r.L;
        CHECK(L.S == S && L.lds_bytes == 8 * (size_t)(40 + 4 * 64 * L.qpl + table_doubles_block(MCSAS_MODEL_SPHERE, r.margs.int_div, 1)));
        printf("%s layout %d %d %#x", id, L.total_slots, L.qpl, L.end_mask);
        for (int s = 0, o = 0; s < S; o += nqs[s++]) { CHECK(L.nq[s] == nqs[s] && L.off[s] == o); printf(" %d %d", L.slots[s], L.pad_off[s]); }
        printf("\n");
    }
    return 0;
}

static int sets_refusals() {
    char id[64];
    for (;;) {
        SetsRequest r(90, {40, 50});
        mcsas_problem &p = r.p;
        if (scanf("%63s %d %d %d %d %d %d %d", id, &p.model_id, &p.n_active, &p.n_devices, &p.positive_background, &p.smear_nk, &p.cache_intensities, &p.exec_mode) != 8) return 0;
        const int rc = r.check();
        printf("%s %d %s\n", id, rc, rc ? g_err.c_str() : "");
    }
}

// (37, 100) points, one of set 1 with sigma == 0: the padded vectors and each set's constants; 65 points in one set: the sums are WeighedData's
static void sets_data() {
    SetsRequest r(137, {37, 100});
    r.sig[40] = 0.;
    CHECK(r.check() == MCSAS_OK && r.L.qpl == 4);
    SetsData d;
    SetsArgs sa;
    memset((void *)&sa, 0xA5, sizeof sa);
    lay_out_sets(&r.p, r.L, &d, &sa);
    CHECK(d.q.size() == 256 && d.w.size() == 256 && d.wI.size() == 256 && d.I.size() == 256);
    CHECK(sa.n_sets == 2 && sa.end_mask == 0x5 && sa.out == nullptr);
    const int first[2] = {0, 37}, count[2] = {37, 100}, at[2] = {0, 64};
    for (int i = 0; i < 256; ++i) {
        const int s = i < 64 ? 0 : 1, k = i - at[s];
        if (i < 192 && k < count[s]) {                                         // entries 0-36 and 64-163: the sets' own points
            const int src = first[s] + k;
            const double e = r.sig[src] == 0. ? 1. : r.sig[src], w = 1. / (e * e);
            CHECK(d.q[i] == r.q[src] && d.I[i] == r.I[src] && d.w[i] == w && d.wI[i] == w * r.I[src]);
        } else {                                                               // 37-63 and 192-255 repeat q[0], 164-191 set 1's first point
            CHECK(d.q[i] == r.q[(i >= 164 && i < 192) ? 37 : 0] && d.w[i] == 0. && d.wI[i] == 0. && d.I[i] == 0.);
        }
    }
    CHECK(d.w[64 + 3] == 1. && d.wI[64 + 3] == r.I[40]);                       // sigma == 0 -> 1
    for (int s = 0; s < MCSAS_MAX_SETS; ++s) {
        const SetConst &c = sa.set[s];
        if (s >= 2) { const SetConst zero{}; CHECK(!memcmp(&c, &zero, sizeof c)); continue; }
        double Sw = 0, SI = 0, SII = 0;
        for (int k = 0; k < count[s]; ++k) { const int i = at[s] + k; Sw += d.w[i]; SI += d.wI[i]; SII += d.wI[i] * d.I[i]; }
        CHECK(c.Sw == Sw && c.SI == SI && c.SII == SII);
        CHECK(c.invSw == 1.0 / c.Sw && c.SIoSw == c.SI / c.Sw && c.Scen == c.SII - c.SI * c.SI / c.Sw && c.nq == (double)count[s]);
    }

    SetsRequest one(65, {65});
    one.sig[9] = 0.;
    CHECK(one.check() == MCSAS_OK && one.L.qpl == 2 && one.L.end_mask == 0x2);
    lay_out_sets(&one.p, one.L, &d, &sa);
    ChainArgs a;
    memset((void *)&a, 0, sizeof a);
    const WeighedData h(&one.p, 128, &a);
    CHECK(!memcmp(&sa.set[0].Sw, &a.Sw, 8) && !memcmp(&sa.set[0].SI, &a.SI, 8) && !memcmp(&sa.set[0].SII, &a.SII, 8));
    CHECK(a.nq == 65 && a.qpad == 128 && d.w == h.w && d.wI == h.wI && d.I == h.I);
}

int main(int argc, char **argv) {
    if (argc > 1 && !strcmp(argv[1], "shapes")) return shapes();
    if (argc > 1 && !strcmp(argv[1], "gate")) return gate();
    if (argc > 1 && !strcmp(argv[1], "sets")) return sets_layouts();
    if (argc > 1 && !strcmp(argv[1], "refusals")) return sets_refusals();
    family_table();
    trace_block();
    tick_budget();
    chain_settings();
    sets_data();
    printf("ok\n");
    return 0;
}
