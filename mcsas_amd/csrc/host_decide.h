// host_decide.h — what libmcsas_hip.so decides without a device (host_decide.hip), beside what host_internal.h declares of that unit
// for every host unit (the refusals, the family table, the trace block's layout): how a problem runs, how a kernel family is launched
// and named, the settings block every chain kernel takes, the request, layout and data of several sets fitted with one population, a
// fetched trace block's transposition, a pipeline launch's ticks.  None of it calls the HIP runtime.
#pragma once
#include "host_internal.h"
#include "chain_sets.h"  // SetsArgs / SetConst only; the kernel is instantiated in kern_wave_sets.hip
#include "chain_wg.h"    // WgGeom / wg_geometry only; the kernels are instantiated in kern_*.hip
#include "pipe_layout.h" // the pipeline's argument blocks, constants and pipe_geometry (no kernel templates)

#pragma GCC visibility push(hidden)

// ------------------------------------------------------------------------------ how a problem runs
int validate_problem(const mcsas_problem *p);
// what the pipeline's tuning word asks for; all zero (automatic) in the release library
struct TuneWord { int rpw = 0, sub = 0, gram_global = 0, eager = 0; };
TuneWord tune_word(const mcsas_problem *p);
// doubles of model tables a block of `waves_per_block` waves keeps in LDS: the shared table and one row scratch per wave
int table_doubles_block(int model_id, int int_div, int waves_per_block);
// How a problem runs: q slots per lane, execution mode, waves per chain, the geometry of the speculative modes and the rows of
// the intensity cache (before the spare row of alloc_rows).  A pure function of its arguments — the caller asks the device for its
// CU count and, where MCSAS_EXEC_AUTO decides, for its free memory (SIZE_MAX: not known, nothing is ruled out by it).
struct PlanShape {
    int qpl = 1, qpad = 0;
    bool wide = false;
    int waves = 1, mode = MCSAS_EXEC_WAVE, cache_rows = 0;
    mcsas::WgGeom wg{};
    mcsas::PipeGeom pipe{};
};
int decide_shape(const mcsas_problem *p, const mcsas::ModelArgs &margs, int n_cus, size_t free_bytes, const TuneWord &tw, PlanShape *s);

// The settings block of a chain kernel's argument block (n_contrib ... conv_crit, the generators, seed and rep_offset) from the
// problem, for every unit that runs chains; find_bg, pos_bg and start_from_min as 0 / 1.  Nothing else of `a` is written.
void fill_chain_settings(const mcsas_problem *p, mcsas::ChainArgs *a);

// ------------------------------------------------------------------------------ one population fitted to several data sets (host_sets.hip runs it)
constexpr int SETS_MAX_SLOTS = Q_MAX_WINDOW / mcsas::WAVE;        // 16 register slots of 64 entries: the largest instance
// Where the sets lie in the padded vectors: set s at [pad_off[s], pad_off[s] + 64 slots[s]), its points at [off[s], off[s] + nq[s]) of
// the caller's; qpl is the smallest instantiated slot count that holds them all, bit j of end_mask marks a set's last slot.
struct SetsLayout {
    int S = 0, qpl = 0, total_slots = 0;
    int nq[MCSAS_MAX_SETS] = {}, off[MCSAS_MAX_SETS] = {}, slots[MCSAS_MAX_SETS] = {}, pad_off[MCSAS_MAX_SETS] = {};
    uint32_t end_mask = 0;
    int scale_mode = 0;                                        // MCSAS_SETS_SCALE_*
    size_t lds_bytes = 0;
};
// Everything mcsas_hip_analyse_sets_mode refuses but a shape without a kernel, in order; fills the layout and the model's argument block.
int check_sets_request(const mcsas_problem *p, int32_t n_sets, const int32_t *set_nq, const mcsas_result *res,
                       const mcsas_sets_result *sets, SetsLayout *L, mcsas::ModelArgs *margs, int32_t scale_mode = MCSAS_SETS_SCALE_PER_SET);
// What mcsas_hip_histogram_sets refuses beyond what mcsas_hip_histogram refuses of the set (host_hist.hip: check_hist_set runs first),
// in order; fills off[s], the first point of set s among the nq points (off[n_sets .. MCSAS_MAX_SETS] = nq).
int check_hist_sets_request(const mcsas_problem *p, int32_t n_sets, const int32_t *set_nq, int32_t scale_mode, int32_t ref_set,
                            uint32_t visible_sets, const mcsas_sets_result *sets, int32_t off[MCSAS_MAX_SETS + 1]);
// The padded vectors, 64 qpl entries each (pad: q of the set's first point — behind the last set, of the first set's —, w = wI = I = 0),
// and what the kernel's second argument holds of the sets: their number, end_mask, the scale mode and each set's SetConst (`out` is the caller's).
struct SetsData { std::vector<double> q, w, wI, I; };
void lay_out_sets(const mcsas_problem *p, const SetsLayout &L, SetsData *d, mcsas::SetsArgs *sa);

// ------------------------------------------------------------------------------ how a kernel family is launched and named
// threads per block of the family's kernel, `waves` being the plan's waves per chain
unsigned family_block(KernelFamily family, int waves);
// A plug-in's kernel of a family: the name expression the run-time compiler instantiates and the key of the program that holds it
// (started and cold kernels are programs of their own, each compiled when first asked for); `given` on a family without a start
// is refused.
int plugin_kernel_name(int model_id, KernelFamily family, int qpl, bool flag, bool given, std::string *expr, std::string *key);

// ------------------------------------------------------------------------------ a fetched trace block, a pipeline launch's ticks
// a slot's block as fetched (TraceLayout: [rep][capacity]) into the caller's [capacity][n_reps] arrays; what lies behind the last
// attempt's out[r].num_moves moves is an earlier attempt's or nothing: -1 / NaN
void trace_transpose(const char *block, size_t R, size_t K, size_t P, const mcsas::ChainOut *out, mcsas_trace *tr);
// The most ticks a pipeline launch enqueues: every attempt runs to max_iter (saturating: max_iter may be 2^62 and a product of two such
// numbers must not wrap to a negative budget).  One attempt: its last window (index ceil(max_iter / Kb) - 1) is scanned at tick
// ceil(max_iter / Kb), exactly; with retries the schedule depends on when attempts end: a generous bound, the host leaves when all are done.
long long pipeline_tick_budget(int64_t max_iter, int32_t max_retries, int kb);

#pragma GCC visibility pop
